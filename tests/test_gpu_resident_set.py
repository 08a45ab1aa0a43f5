"""fosvos_augment_sample and the device-resident offline training set on a real MI355X: the kernel against
custom_transforms.resize (the numpy restatement the per-iteration DataLoader runs) bit for bit, its argument checks, the
loader against that DataLoader draw for draw, and train_offline._train fed by either loader."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))

from dataloaders import custom_transforms as T  # noqa: E402
from dataloaders.davis_2016 import DAVIS2016, MEANVAL  # noqa: E402
from test_resident_set_cpu import N_EPOCHS, _epochs, assert_same_epochs, write_davis_tree  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
_TABLES = (("col_taps", np.int32), ("col_w", np.float32), ("row_taps", np.int32), ("row_w", np.float32),
           ("col_near", np.int32), ("row_near", np.int32))


def _dataset():
    ds = DAVIS2016.__new__(DAVIS2016)
    ds.meanval = MEANVAL
    return ds


def _luts(ds, lab):
    ramp = np.repeat(np.arange(256, dtype=np.uint8)[:, None, None], 3, axis=2)
    img_lut = torch.from_numpy(np.ascontiguousarray(ds.convert_raw(ramp, None)[0].reshape(256, 3))).to(DEV)
    gt_lut = torch.from_numpy(np.arange(256, dtype=np.float32) / np.float32(max(float(lab.max()), 1e-8))).to(DEV)
    return img_lut, gt_lut


def _on_device(arr, offset):
    """A uint8 array on the device, ``offset`` bytes into its buffer (rows that start at any alignment)."""
    flat = torch.zeros(arr.size + offset + 32, dtype=torch.uint8, device=DEV)
    view = flat[offset:offset + arr.size]
    view.copy_(torch.from_numpy(np.ascontiguousarray(arr).reshape(-1)))
    return view.view(arr.shape)


def _run_kernel(img, lab, flip, sc, offset=0):
    from fosvos_hip import ops
    h, w = lab.shape
    plan = T.resize_plan(h, w, sc, sc)
    tables = None if plan["copy"] else tuple(
        torch.from_numpy(np.ascontiguousarray(plan[k], dtype=dt)).to(DEV) for k, dt in _TABLES)
    img_lut, gt_lut = _luts(_dataset(), lab)
    frame, mask = _on_device(img, offset), _on_device(lab, offset + 5)
    image = torch.full((1, 3, plan["oh"], plan["ow"]), float("nan"), device=DEV)
    gt = torch.full((1, 1, plan["oh"], plan["ow"]), float("nan"), device=DEV)
    ops.augment_sample(frame, mask, flip, img_lut, gt_lut, image, gt, tables)
    return image, gt


@pytest.mark.parametrize("size,offset", [((480, 854), 0), ((61, 107), 3), ((24, 40), 13), ((480, 854), 7)])
def test_kernel_is_the_numpy_resize_bit_for_bit(size, offset):
    h, w = size
    ds = _dataset()
    rng = np.random.RandomState(h + w)
    img = rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    lab = np.where(rng.rand(h, w) > 0.5, 255, 0).astype(np.uint8)
    lab[h // 3:, : w // 2] = 128
    side = torch.cuda.Stream(DEV)
    for sc in (0.5, 0.8, 1):
        for flip in (False, True):
            image, gt = ds.convert_raw(img, lab)
            if flip:
                image, gt = np.ascontiguousarray(image[:, ::-1]), np.ascontiguousarray(gt[:, ::-1])
            want = T.ToTensor()({"image": T.resize(image, sc, sc), "gt": T.resize(gt, sc, sc)})
            with torch.cuda.stream(side):  # the launch goes to the caller's (current) stream
                got_img, got_gt = _run_kernel(img, lab, flip, sc, offset)
            side.synchronize()
            for key, got in (("image", got_img), ("gt", got_gt)):
                ref = want[key].unsqueeze(0)
                assert tuple(got.shape) == tuple(ref.shape), (key, sc, flip)
                got = got.cpu()
                assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), \
                    (key, size, sc, flip, (got - ref).abs().max().item())


def test_bad_arguments_raise_before_any_launch():
    from fosvos_hip import FosvosHipError, lib, ops
    h, w = 24, 40
    plan = T.resize_plan(h, w, 0.5, 0.5)
    tables = tuple(torch.from_numpy(np.ascontiguousarray(plan[k], dtype=dt)).to(DEV) for k, dt in _TABLES)
    frame = torch.zeros((h, w, 3), dtype=torch.uint8, device=DEV)
    mask = torch.zeros((h, w), dtype=torch.uint8, device=DEV)
    img_lut, gt_lut = torch.zeros((256, 3), device=DEV), torch.zeros(256, device=DEV)
    image, gt = torch.zeros((1, 3, 12, 20), device=DEV), torch.zeros((1, 1, 12, 20), device=DEV)
    ops.augment_sample(frame, mask, False, img_lut, gt_lut, image, gt, tables)  # the good call
    with pytest.raises(TypeError):
        ops.augment_sample(frame.float(), mask, False, img_lut, gt_lut, image, gt, tables)
    with pytest.raises(TypeError):
        ops.augment_sample(frame, mask, False, img_lut, gt_lut, image.double(), gt, tables)
    with pytest.raises(TypeError):
        ops.augment_sample(frame, mask, False, img_lut, gt_lut, image, gt, (tables[0].long(),) + tables[1:])
    with pytest.raises(RuntimeError):
        ops.augment_sample(frame.cpu(), mask, False, img_lut, gt_lut, image, gt, tables)
    with pytest.raises(RuntimeError):
        ops.augment_sample(frame, mask, False, img_lut.cpu(), gt_lut, image, gt, tables)
    with pytest.raises(ValueError):
        ops.augment_sample(frame.transpose(0, 1), mask, False, img_lut, gt_lut, image, gt, tables)
    with pytest.raises(ValueError):
        ops.augment_sample(frame, mask, False, img_lut, gt_lut, torch.zeros((1, 3, 20, 12), device=DEV).transpose(2, 3),
                           gt, tables)
    with pytest.raises(ValueError):  # a size change needs the tables
        ops.augment_sample(frame, mask, False, img_lut, gt_lut, image, gt, None)
    with pytest.raises(ValueError):  # tables of another output size
        ops.augment_sample(frame, mask, False, img_lut, gt_lut, torch.zeros((1, 3, 19, 32), device=DEV),
                           torch.zeros((1, 1, 19, 32), device=DEV), tables)
    # the C entry point refuses a partial table set and an over-wide frame on its own
    rc = lib().fosvos_augment_sample(frame.data_ptr(), mask.data_ptr(), h, w, 0, tables[0].data_ptr(), None, None, None,
                                     None, None, 12, 20, img_lut.data_ptr(), gt_lut.data_ptr(), image.data_ptr(),
                                     gt.data_ptr(), 0, None)
    assert rc == -2 and b"six" in lib().fosvos_last_error()
    wide = torch.zeros((1, 5000, 3), dtype=torch.uint8, device=DEV)  # (buffers that would hold it, all the same)
    wide_out = torch.zeros((1, 3, 1, 5000), device=DEV)
    rc = lib().fosvos_augment_sample(wide.data_ptr(), wide.data_ptr(), 1, 5000, 0, None, None, None, None, None, None,
                                     1, 5000, img_lut.data_ptr(), gt_lut.data_ptr(), wide_out.data_ptr(),
                                     wide_out.data_ptr(), 0, None)
    assert rc == -1 and b"W <= 4096" in lib().fosvos_last_error()
    with pytest.raises(FosvosHipError):
        ops.check(rc, "augment_sample")
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def davis_root(tmp_path_factory):
    return write_davis_tree(tmp_path_factory.mktemp("davis_set_gpu"))


@pytest.mark.parametrize("shard", [None, (0, 2), (1, 2)])
def test_device_loader_replays_the_dataloader(davis_root, shard):
    from util import io_helper
    from dataloaders.resident import ResidentTrainSetLoader
    runs = []
    for resident_set in (False, True):
        torch.manual_seed(31)
        loader = io_helper.get_data_loader_train(str(davis_root), 1, shard=shard, resident_set=resident_set)
        assert isinstance(loader, ResidentTrainSetLoader) == resident_set
        if resident_set:
            assert loader.device.type == "cuda" and loader.device_bytes > 0
        runs.append(_epochs(loader, N_EPOCHS, set_epoch=shard is not None))
    for ep in runs[1][0]:
        assert all(m["image"].is_cuda and m["gt"].is_cuda for m in ep)
    assert_same_epochs(*runs)


class _Prov:
    name = "vgg16"

    def __init__(self, net):
        self.network = net

    def save_model(self, *a, **k):
        pass


class _Writer:
    def add_scalar(self, *a, **k):
        pass

    def close(self):
        pass


def _train_once(root, resident_set):
    import train_offline
    from networks.osvos_vgg import OSVOS_VGG
    from oracle import osvos_ref as O
    from util import io_helper
    from util.network_provider import VGGOfflineProvider
    net = OSVOS_VGG(pretrained=0)
    net.load_state_dict(O.make_state_dict(6))
    prov = VGGOfflineProvider.__new__(VGGOfflineProvider)
    prov.network = net.to(DEV)
    opt = prov.get_optimizer(learning_rate=1e-6)
    torch.manual_seed(2024)
    loader = io_helper.get_data_loader_train(str(root), 1, resident_set=resident_set)
    train_offline.data_parallel = False
    ret = train_offline._train(_Prov(prov.network), loader, None, opt, _Writer(), 0, 3, 2, 10 ** 9, False, 5)
    assert ret["iterations"] == 3 * 6
    return ret["losses_train"], {k: v.detach().cpu().clone() for k, v in prov.network.state_dict().items()}


def test_offline_training_is_the_same_with_either_loader(tmp_path):
    """train_offline._train (3 epochs of 6 samples, a step every 2) from the same seed and weights: the per-epoch losses and
    the final state_dict of the run fed by the resident set equal those of the DataLoader-fed run.  The bar is the spread
    of two DataLoader-fed runs (zero when the step is run-to-run bit-deterministic)."""
    root = write_davis_tree(tmp_path, seqs={"a": (2, 80, 120), "b": (2, 80, 120), "c": (2, 80, 120)},
                            train=["a", "b", "c"])
    base = _train_once(root, False)
    again = _train_once(root, False)
    resident = _train_once(root, True)

    def spread(x, y):
        loss = max(abs(a - b) for ea, eb in zip(x[0], y[0]) for a, b in zip(ea, eb))
        weights = max((x[1][k] - y[1][k]).abs().max().item() for k in x[1])
        return loss, weights

    bar = spread(base, again)
    got = spread(base, resident)
    print(f"DataLoader vs DataLoader {bar}, DataLoader vs resident {got}")
    assert len(resident[0]) == 3
    assert got[0] <= bar[0] and got[1] <= bar[1], (got, bar)
    from oracle import osvos_ref as O
    init = O.make_state_dict(6)
    assert max((resident[1][k] - init[k]).abs().max().item() for k in resident[1]) > 0  # the weights did train
