"""fosvos_warp_sample and the rotating resident loaders on a real MI355X: the kernel against custom_transforms.warp_affine
(and the reference's renormalisation) bit for bit, its refusals, both loaders against the host DataLoader draw for draw, and
train_online._train fed by either.  No tolerance anywhere."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))

from dataloaders import custom_transforms as T  # noqa: E402
from dataloaders.davis_2016 import DAVIS2016, MEANVAL  # noqa: E402
from fosvos_hip.options import RotateOptions  # noqa: E402
from test_augment_rotate_cpu import FORMS, ROTATIONS, SEQS, TRAIN, assert_same_one_shot_epochs, sample_bytes  # noqa: E402
from test_resident_set_cpu import N_EPOCHS, _epochs, assert_same_epochs, write_davis_tree  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
IDENTITY = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
FAR = np.array([[1.0, 0.0, 1000.0], [0.0, 1.0, 1000.0]])
SHEAR = np.array([[1.0, 0.3, -4.5], [-0.2, 1.1, 3.25]])  # taps fall outside on all four sides


def _dataset():
    ds = DAVIS2016.__new__(DAVIS2016)
    ds.meanval = MEANVAL
    return ds


def _luts(ds, lab):
    ramp = np.repeat(np.arange(256, dtype=np.uint8)[:, None, None], 3, axis=2)
    img_lut = np.ascontiguousarray(ds.convert_raw(ramp, None)[0].reshape(256, 3))
    gt_lut = np.arange(256, dtype=np.float32) / np.float32(max(float(lab.max()), 1e-8))
    return img_lut, gt_lut


def _on_device(arr, offset):
    """A uint8 array on the device, ``offset`` bytes into its buffer (rows that start at any alignment)."""
    flat = torch.zeros(arr.size + offset + 32, dtype=torch.uint8, device=DEV)
    view = flat[offset:offset + arr.size]
    view.copy_(torch.from_numpy(np.ascontiguousarray(arr).reshape(-1)))
    return view.view(arr.shape)


def _renormalized(tmp):
    """The two steps of the reference's ScaleNRotate behind its warp."""
    if tmp.min() < 0.0:
        tmp = tmp - tmp.min()
    if tmp.max() > 1.0:
        tmp = tmp / tmp.max()
    return tmp


def _matrices(h, w):
    return [("rot%g_%g" % rs, T.rotation_matrix((w / 2, h / 2), *rs)) for rs in ROTATIONS] + \
        [("identity", IDENTITY), ("far", FAR), ("shear", SHEAR)]


@pytest.mark.parametrize("size,offset", [((13, 17), 0), ((24, 40), 13), ((61, 107), 3), ((33, 130), 7)])
def test_kernel_is_the_numpy_warp_bit_for_bit(size, offset):
    from fosvos_hip import ops
    h, w = size
    ds = _dataset()
    side = torch.cuda.Stream(DEV)
    need = ops.warp_workspace_bytes(h, w)
    assert need == 8 * ((w + 63) // 64) * ((h + 3) // 4)
    for peak in (255, 1):
        img, lab = sample_bytes(h, w, peak)
        if peak == 1:
            lab = (lab > 0).astype(np.uint8)
        assert lab.max() == peak
        img_lut, gt_lut = _luts(ds, lab)
        frame, mask = _on_device(img, offset), _on_device(lab, offset + 5)
        d_img_lut, d_gt_lut = torch.from_numpy(img_lut).to(DEV), torch.from_numpy(gt_lut).to(DEV)
        for name, matrix in _matrices(h, w):
            for flip in (False, True):
                image, gt = ds.convert_raw(img, lab)
                if flip:
                    image, gt = np.ascontiguousarray(image[:, ::-1]), np.ascontiguousarray(gt[:, ::-1])
                warped = {"image": T.warp_affine(image, matrix), "gt": T.warp_affine(gt, matrix)}
                if name == "identity":  # the LUT copy
                    cols = np.arange(w)[::-1] if flip else np.arange(w)
                    assert np.array_equal(warped["image"], img_lut[img[:, cols], np.arange(3)[None, None, :]])
                    assert np.array_equal(warped["gt"], gt_lut[lab[:, cols]])
                if name == "far":
                    assert not warped["image"].any() and not warped["gt"].any()
                for renormalize in (False, True):
                    want = {k: (_renormalized(v) if renormalize else v) for k, v in warped.items()}
                    assert np.array_equal(want["gt"], warped["gt"])  # on a mask the renormalisation is a no-op
                    want = T.ToTensor()(want)
                    got_img = torch.full((1, 3, h, w), float("nan"), device=DEV)
                    got_gt = torch.full((1, 1, h, w), float("nan"), device=DEV)
                    ws = torch.full((need + 4,), 0xFF, dtype=torch.uint8, device=DEV) if renormalize else None
                    with torch.cuda.stream(side):  # the launches go to the caller's (current) stream
                        ops.warp_sample(frame, mask, flip, matrix, d_img_lut, d_gt_lut, got_img, got_gt,
                                        renormalize=renormalize, workspace=None if ws is None else ws[:need])
                    side.synchronize()
                    for key, got in (("image", got_img), ("gt", got_gt)):
                        ref, got = want[key].unsqueeze(0), got.cpu()
                        assert tuple(got.shape) == tuple(ref.shape) and got.dtype == ref.dtype
                        bad = got.view(torch.int32) != ref.view(torch.int32)
                        assert not bad.any(), (key, size, peak, name, flip, renormalize, int(bad.sum()),
                                               got[bad][:4].tolist(), ref[bad][:4].tolist())
                    if ws is not None:
                        assert bool((ws[need:] == 0xFF).all())  # nothing behind the reported size is written


class _Counting:
    """fosvos_hip.lib() with the warp launches counted."""

    def __init__(self, real):
        self.real, self.launches = real, 0

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if name != "fosvos_warp_sample":
            return fn

        def call(*args):
            self.launches += 1
            return fn(*args)
        return call


def test_bad_arguments_raise_before_any_launch(monkeypatch):
    from fosvos_hip import FosvosHipError, lib, ops
    h, w = 24, 40
    frame = torch.zeros((h, w, 3), dtype=torch.uint8, device=DEV)
    mask = torch.zeros((h, w), dtype=torch.uint8, device=DEV)
    img_lut, gt_lut = torch.zeros((256, 3), device=DEV), torch.zeros(256, device=DEV)
    image, gt = torch.zeros((1, 3, h, w), device=DEV), torch.zeros((1, 1, h, w), device=DEV)
    ws = torch.zeros(ops.warp_workspace_bytes(h, w), dtype=torch.uint8, device=DEV)
    m = T.rotation_matrix((w / 2, h / 2), 30, 0.75)
    counting = _Counting(lib())
    monkeypatch.setattr(ops, "lib", lambda: counting)

    def call(frame=frame, mask=mask, flip=False, matrix=m, img_lut=img_lut, gt_lut=gt_lut, image=image, gt=gt, **kw):
        ops.warp_sample(frame, mask, flip, matrix, img_lut, gt_lut, image, gt, **kw)

    call()
    call(renormalize=True, workspace=ws)
    call(matrix=m.tolist())
    assert counting.launches == 3
    for error, kw in (
            (TypeError, dict(frame=frame.float())), (TypeError, dict(mask=mask.int())), (TypeError, dict(image=image.double())),
            (TypeError, dict(gt=gt.half())), (TypeError, dict(img_lut=img_lut.double())), (TypeError, dict(gt_lut=gt_lut.long())),
            (TypeError, dict(renormalize=True, workspace=ws.view(torch.int8))),
            (RuntimeError, dict(frame=frame.cpu())), (RuntimeError, dict(img_lut=img_lut.cpu())), (RuntimeError, dict(gt=gt.cpu())),
            (RuntimeError, dict(renormalize=True, workspace=ws.cpu())),
            (ValueError, dict(frame=torch.zeros((w, h, 3), dtype=torch.uint8, device=DEV).transpose(0, 1))),
            (ValueError, dict(image=torch.zeros((1, 3, w, h), device=DEV).transpose(2, 3))),
            (ValueError, dict(frame=torch.zeros((h, w, 4), dtype=torch.uint8, device=DEV))),
            (ValueError, dict(mask=torch.zeros((h, w + 1), dtype=torch.uint8, device=DEV))),
            (ValueError, dict(image=torch.zeros((1, 3, h // 2, w // 2), device=DEV))),  # a warp keeps the size
            (ValueError, dict(gt=torch.zeros((1, 1, h, w + 1), device=DEV))),
            (ValueError, dict(gt=torch.zeros((1, h, w), device=DEV))),
            (ValueError, dict(img_lut=torch.zeros((3, 256), device=DEV))), (ValueError, dict(gt_lut=torch.zeros(255, device=DEV))),
            (ValueError, dict(matrix=np.zeros((2, 3)))),                                  # singular
            (ValueError, dict(matrix=[[1.0, 2.0, 0.0], [2.0, 4.0, 0.0]])),                  # singular
            (ValueError, dict(matrix=[[1.0, 0.0, float("nan")], [0.0, 1.0, 0.0]])),
            (ValueError, dict(matrix=[[float("inf"), 0.0, 0.0], [0.0, 1.0, 0.0]])),
            (ValueError, dict(matrix=np.eye(3))), (ValueError, dict(matrix=[1.0, 0.0, 0.0])), (ValueError, dict(matrix="rot")),
            (ValueError, dict(renormalize=True)),                                         # no workspace
            (ValueError, dict(renormalize=True, workspace=ws[:-1])),                      # too small
            (ValueError, dict(renormalize=True, workspace=torch.zeros(ws.numel() + 8, dtype=torch.uint8, device=DEV)[1:])),
            (ValueError, dict(renormalize=1, workspace=ws))):
        with pytest.raises(error, match="warp_sample"):
            call(**kw)
    assert counting.launches == 3
    for bad in ((0, 4), (4, 0), (8193, 4), (4, 8193), (True, 4), (4.0, 4)):
        with pytest.raises(ValueError, match="warp_workspace_bytes"):
            ops.warp_workspace_bytes(*bad)
    # a matrix the op layer takes (finite, invertible) and the entry refuses: the call is made, nothing is launched
    with pytest.raises(FosvosHipError, match="2\\^30"):
        call(matrix=[[1e-12, 0.0, 0.0], [0.0, 1e-12, 0.0]])
    assert counting.launches == 4

    # the C entry's own refusals
    L = lib()
    E_SHAPE, E_ARG, E_WORKSPACE = -1, -2, -3

    def entry(H=h, W=w, coeff=(1.0, 0.0, 0.0, 0.0, 1.0, 0.0), renormalize=0, workspace=None, workspace_bytes=0):
        return L.fosvos_warp_sample(frame.data_ptr(), mask.data_ptr(), H, W, 0, *coeff, img_lut.data_ptr(), gt_lut.data_ptr(),
                                    image.data_ptr(), gt.data_ptr(), renormalize, workspace, workspace_bytes, 0, None)

    for coeff in ((float("nan"), 0.0, 0.0, 0.0, 1.0, 0.0), (1.0, 0.0, float("inf"), 0.0, 1.0, 0.0),
                  (1.0, 0.0, 0.0, 0.0, float("-inf"), 0.0)):
        assert entry(coeff=coeff) == E_ARG and b"non-finite coefficient" in L.fosvos_last_error()
    for coeff in ((1.0, 0.0, 2.0 ** 30 + 1, 0.0, 1.0, 0.0), (1.0, 0.0, 0.0, 0.0, 1.0, -(2.0 ** 30) - 1),
                  (2.0 ** 30, 0.0, 0.0, 0.0, 1.0, 0.0), (1.0, 0.0, 0.0, 1.0, -(2.0 ** 30), 0.0), (1e300, 0.0, 0.0, 0.0, 1.0, 0.0)):
        assert entry(coeff=coeff) == E_ARG and b"beyond +-2^30" in L.fosvos_last_error(), coeff
    for H, W in ((h, 8193), (8193, w), (0, w), (h, -1)):  # (checked before anything is read)
        assert entry(H=H, W=W) == E_SHAPE and b"<= 8192" in L.fosvos_last_error()
        assert L.fosvos_warp_workspace_bytes(H, W) == 0
    assert entry(renormalize=1) == E_WORKSPACE and b"renormalize needs a workspace" in L.fosvos_last_error()
    assert entry(renormalize=1, workspace=ws.data_ptr(), workspace_bytes=ws.numel() - 1) == E_WORKSPACE
    assert L.fosvos_warp_sample(None, mask.data_ptr(), h, w, 0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, img_lut.data_ptr(),
                                gt_lut.data_ptr(), image.data_ptr(), gt.data_ptr(), 0, None, 0, 0, None) == E_ARG
    with pytest.raises(FosvosHipError):
        ops.check(E_WORKSPACE, "warp_sample")
    assert L.fosvos_warp_workspace_bytes(8192, 8192) == 8 * 128 * 2048 and L.fosvos_warp_workspace_bytes(1, 1) == 8
    assert entry(coeff=(1.0, 0.0, 2.0 ** 30 - w, 0.0, 1.0, -(2.0 ** 30))) == 0  # at the bound: taken (and all zeros)
    torch.cuda.synchronize()
    assert not image.any() and not gt.any()


# ------------------------------------------------------------------------------------------ the loaders on the device
@pytest.fixture(scope="module")
def davis_root(tmp_path_factory):
    return write_davis_tree(tmp_path_factory.mktemp("davis_rotate_gpu"), seqs=SEQS, train=TRAIN)


@pytest.mark.parametrize("form", sorted(FORMS))
def test_device_one_shot_loader_replays_the_dataloader(davis_root, form):
    from util import io_helper
    from dataloaders.resident import ResidentOneShotLoader
    runs = []
    for resident in (False, True):
        torch.manual_seed(31)
        loader = io_helper.get_data_loader_train(str(davis_root), 1, "camel", resident=resident, rotate=FORMS[form])
        assert isinstance(loader, ResidentOneShotLoader) == resident
        if resident:
            assert loader.device.type == "cuda" and loader._frame.is_cuda and loader._frame.dtype == torch.uint8
        runs.append(_epochs(loader, N_EPOCHS))
    assert all(ep[0]["image"].is_cuda and ep[0]["gt"].is_cuda for ep in runs[1][0])
    assert_same_one_shot_epochs(*runs)
    assert len(loader.draws) == N_EPOCHS


@pytest.mark.parametrize("form,shard", [("tuple", None), ("tuple", (0, 2)), ("tuple", (1, 2)), ("list", None)])
def test_device_set_loader_replays_the_dataloader(davis_root, form, shard):
    from util import io_helper
    from dataloaders.resident import ResidentTrainSetLoader
    runs = []
    for resident_set in (False, True):
        torch.manual_seed(31)
        loader = io_helper.get_data_loader_train(str(davis_root), 1, shard=shard, resident_set=resident_set, rotate=FORMS[form])
        assert isinstance(loader, ResidentTrainSetLoader) == resident_set
        if resident_set:
            assert loader.device.type == "cuda" and loader.device_bytes > 0 and not loader._plans
            assert (loader._workspace is not None) == FORMS[form].renormalize
        runs.append(_epochs(loader, N_EPOCHS, set_epoch=shard is not None))
    for ep in runs[1][0]:
        assert all(m["image"].is_cuda and m["gt"].is_cuda for m in ep)
    assert_same_epochs(*runs)


# ------------------------------------------------------------------------------------------ the loop
EPOCHS = 4


class _Writer:
    def add_scalar(self, *a, **k):
        pass

    def close(self):
        pass


def _train_once(root, resident, rotate):
    import train_online
    from networks.osvos_vgg import OSVOS_VGG
    from oracle import osvos_ref as O
    from util import io_helper
    from util.network_provider import VGGOnlineProvider
    net = OSVOS_VGG(pretrained=0)
    net.load_state_dict(O.make_state_dict(6))
    prov = VGGOnlineProvider.__new__(VGGOnlineProvider)
    prov.name = "vgg16"
    prov.network = net.to(DEV)
    prov.save_model = lambda *a, **k: None
    opt = prov.get_optimizer(learning_rate=1e-6)
    torch.manual_seed(2024)
    loader = io_helper.get_data_loader_train(str(root), 1, "a", resident=resident, rotate=rotate)
    train_online.data_parallel = False
    ret = train_online._train(prov, loader, opt, _Writer(), "a", 0, EPOCHS, 2, 10 ** 9)
    assert ret["iterations"] == EPOCHS
    if resident:
        assert len(loader.draws) == EPOCHS and len({d[1:] for d in loader.draws}) == EPOCHS
    return ret["loss"], {k: v.detach().cpu().clone() for k, v in prov.network.state_dict().items()}


def test_online_training_is_the_same_with_either_loader(tmp_path):
    """train_online._train (4 epochs of the one sample, a step every 2) from the same seed and weights: the logged losses and
    the final state_dict of the run fed by the rotating resident loader equal those of the run fed by the rotating
    DataLoader.  The bar is the spread of two DataLoader-fed runs (zero when the step is run-to-run bit-deterministic)."""
    root = write_davis_tree(tmp_path, seqs={"a": (2, 80, 120)}, train=["a"])
    rotate = RotateOptions()
    base = _train_once(root, False, rotate)
    again = _train_once(root, False, rotate)
    resident = _train_once(root, True, rotate)

    def spread(x, y):
        loss = max(abs(a - b) for a, b in zip(x[0], y[0]))
        weights = max((x[1][k] - y[1][k]).abs().max().item() for k in x[1])
        return loss, weights

    bar = spread(base, again)
    got = spread(base, resident)
    print(f"DataLoader vs DataLoader {bar}, DataLoader vs resident {got}")
    assert len(resident[0]) == len(base[0]) == EPOCHS
    assert got[0] <= bar[0] and got[1] <= bar[1], (got, bar)
    from oracle import osvos_ref as O
    init = O.make_state_dict(6)
    assert max((resident[1][k] - init[k]).abs().max().item() for k in resident[1]) > 0  # the weights did train
