"""fosvos_lucid_sample and the lucid one-shot loader on a real MI355X: the kernel against dataloaders/lucid.compose bit for
bit, its refusals, the loader on the device against the same loader on the CPU draw for draw, and train_online._train fed by
it with one launch per draw.  No tolerance anywhere."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))

from dataloaders import lucid as L  # noqa: E402
from dataloaders.davis_2016 import DAVIS2016  # noqa: E402
from fosvos_hip.options import LucidOptions  # noqa: E402
from test_augment_lucid_cpu import (FAR, IDENTITY, N_EPOCHS, ONE, SEQS, SHEAR, ZERO, drawn_pairs, lucid_epochs, luts,  # noqa: E402
                                    sample)
from test_resident_set_cpu import write_davis_tree  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GAIN, BIAS = np.array([1.1, 0.9, 1.05], np.float32), np.array([3.0, -2.0, 0.5], np.float32)


def _on_device(arr, offset):
    """A uint8 array on the device, ``offset`` bytes into its buffer (rows that start at any alignment)."""
    flat = torch.zeros(arr.size + offset + 32, dtype=torch.uint8, device=DEV)
    view = flat[offset:offset + arr.size]
    view.copy_(torch.from_numpy(np.ascontiguousarray(arr).reshape(-1)))
    return view.view(arr.shape)


def _pairs(h, w, mask, flip):
    """(name, M_bg, M_fg, gain, bias): the fixed pairs, then three drawn as the loader draws them."""
    fixed = [("identity/identity", IDENTITY, IDENTITY, ONE, ZERO), ("identity/far", IDENTITY, FAR, GAIN, BIAS),
             ("shear/identity", SHEAR, IDENTITY, GAIN, BIAS), ("identity/shear", IDENTITY, SHEAR, ONE, BIAS),
             ("shear/shear", SHEAR, SHEAR, GAIN, ZERO), ("shear/none", SHEAR, None, GAIN, BIAS)]
    drawn = [("drawn%d" % k,) + p for k, p in enumerate(drawn_pairs(h, w, mask, flip)) if p[1] is not None]
    return fixed + drawn


def _check(ops, side, arrays, tables, offset, flip, pair, tag):
    frame, background, mask = arrays
    img_lut, gt_lut = tables
    name, m_bg, m_fg, gain, bias = pair
    h, w = mask.shape
    want_img, want_gt = L.compose(frame, background, mask, img_lut, gt_lut, flip, m_bg, m_fg, gain, bias)
    d = [_on_device(frame, offset), _on_device(background, offset + 2), _on_device(mask, offset + 5)]
    d_img_lut, d_gt_lut = torch.from_numpy(img_lut).to(DEV), torch.from_numpy(gt_lut).to(DEV)
    got_img = torch.full((1, 3, h, w), float("nan"), device=DEV)
    got_gt = torch.full((1, 1, h, w), float("nan"), device=DEV)
    with torch.cuda.stream(side):  # the launch goes to the caller's (current) stream
        ops.lucid_sample(*d, flip, m_bg, m_fg, gain, bias, d_img_lut, d_gt_lut, got_img, got_gt)
    side.synchronize()
    for key, got, ref in (("image", got_img[0].permute(1, 2, 0), want_img), ("gt", got_gt[0, 0], want_gt)):
        got = got.contiguous().cpu().numpy()
        assert got.shape == ref.shape and got.dtype == ref.dtype
        bad = got.view(np.uint32) != ref.view(np.uint32)
        assert not bad.any(), (key, tag, name, flip, int(bad.sum()), got[bad][:4].tolist(), ref[bad][:4].tolist())
    return want_img, want_gt


@pytest.mark.parametrize("size,offset", [((13, 17), 0), ((24, 40), 13), ((61, 107), 3), ((33, 130), 7)])
def test_kernel_is_the_numpy_composition_bit_for_bit(size, offset):
    from fosvos_hip import ops
    h, w = size
    side = torch.cuda.Stream(DEV)
    for peak in (255, 1):
        arrays = sample(h, w, peak)
        assert arrays[2].max() == peak
        tables = luts(arrays[2])
        for flip in (False, True):
            blended = 0
            for pair in _pairs(h, w, arrays[2], flip):
                _, want_gt = _check(ops, side, arrays, tables, offset, flip, pair, (size, peak))
                if pair[0].startswith("drawn"):
                    fmask = arrays[2][:, ::-1] if flip else arrays[2]
                    alpha = L.object_alpha(fmask, pair[2])
                    blended += int(((alpha > 0) & (alpha < 1)).sum())
                    assert (alpha == 1).any() and (alpha == 0).any() and want_gt.any()
            assert blended > 0  # all three branches of a pixel were taken
    # an empty mask, a full mask and a mask whose box touches two borders
    for kind in ("empty", "full", "corner"):
        arrays = sample(h, w, 255, kind)
        tables = luts(arrays[2])
        for flip in (False, True):
            for pair in _pairs(h, w, arrays[2], flip)[1:]:
                _check(ops, side, arrays, tables, offset, flip, pair, (size, kind))


class _Counting:
    """fosvos_hip.lib() with the lucid launches counted."""

    def __init__(self, real):
        self.real, self.launches = real, 0

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if name != "fosvos_lucid_sample":
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
    counting = _Counting(lib())
    monkeypatch.setattr(ops, "lib", lambda: counting)

    def call(frame=frame, background=frame, mask=mask, flip=False, matrix_bg=SHEAR, matrix_fg=IDENTITY, gain=GAIN, bias=BIAS,
             img_lut=img_lut, gt_lut=gt_lut, image=image, gt=gt):
        ops.lucid_sample(frame, background, mask, flip, matrix_bg, matrix_fg, gain, bias, img_lut, gt_lut, image, gt)

    call()
    call(matrix_fg=None, gain=[1, 2, 3], bias=(0.0, 0.0, 0.0))
    call(matrix_bg=SHEAR.tolist())
    assert counting.launches == 3
    nan, inf = float("nan"), float("inf")
    for error, kw in (
            (TypeError, dict(frame=frame.float())), (TypeError, dict(background=frame.int())), (TypeError, dict(mask=mask.int())),
            (TypeError, dict(image=image.double())), (TypeError, dict(gt=gt.half())), (TypeError, dict(img_lut=img_lut.double())),
            (TypeError, dict(gt_lut=gt_lut.long())),
            (RuntimeError, dict(frame=frame.cpu())), (RuntimeError, dict(background=frame.cpu())),
            (RuntimeError, dict(img_lut=img_lut.cpu())), (RuntimeError, dict(gt=gt.cpu())),
            (ValueError, dict(frame=torch.zeros((w, h, 3), dtype=torch.uint8, device=DEV).transpose(0, 1))),
            (ValueError, dict(frame=torch.zeros((h, w, 4), dtype=torch.uint8, device=DEV))),
            (ValueError, dict(background=torch.zeros((h, w + 1, 3), dtype=torch.uint8, device=DEV))),
            (ValueError, dict(mask=torch.zeros((h, w + 1), dtype=torch.uint8, device=DEV))),
            (ValueError, dict(image=torch.zeros((1, 3, h // 2, w // 2), device=DEV))),
            (ValueError, dict(gt=torch.zeros((1, 1, h, w + 1), device=DEV))), (ValueError, dict(gt=torch.zeros((1, h, w), device=DEV))),
            (ValueError, dict(img_lut=torch.zeros((3, 256), device=DEV))), (ValueError, dict(gt_lut=torch.zeros(255, device=DEV))),
            (ValueError, dict(matrix_bg=np.zeros((2, 3)))), (ValueError, dict(matrix_fg=[[1.0, 2.0, 0.0], [2.0, 4.0, 0.0]])),
            (ValueError, dict(matrix_bg=[[1.0, 0.0, nan], [0.0, 1.0, 0.0]])), (ValueError, dict(matrix_fg=[[inf, 0.0, 0.0], [0.0, 1.0, 0.0]])),
            (ValueError, dict(matrix_bg=np.eye(3))), (ValueError, dict(matrix_fg="shift")), (ValueError, dict(matrix_bg=None)),
            (ValueError, dict(gain=[1.0, nan, 1.0])), (ValueError, dict(bias=[0.0, 0.0, inf])), (ValueError, dict(gain=[1.0, 1.0])),
            (ValueError, dict(bias=1.0)), (ValueError, dict(gain=[1e39, 1.0, 1.0])), (ValueError, dict(bias="dark"))):
        with pytest.raises(error, match="lucid_sample"):
            call(**kw)
    assert counting.launches == 3
    # matrices the op layer takes (finite, invertible) and the entry refuses: the call is made, nothing is launched
    tiny = [[1e-12, 0.0, 0.0], [0.0, 1e-12, 0.0]]
    with pytest.raises(FosvosHipError, match="background matrix, beyond \\+-2\\^30"):
        call(matrix_bg=tiny)
    with pytest.raises(FosvosHipError, match="object matrix, beyond \\+-2\\^30"):
        call(matrix_fg=tiny)
    assert counting.launches == 5

    # the C entry's own refusals
    Lib = lib()
    E_SHAPE, E_ARG = -1, -2
    eye = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)

    def entry(H=h, W=w, bg=eye, fg=eye, fg_on=1, gains=(1.0, 1.0, 1.0), biases=(0.0, 0.0, 0.0), frame_ptr=frame.data_ptr()):
        return Lib.fosvos_lucid_sample(frame_ptr, frame.data_ptr(), mask.data_ptr(), H, W, 0, *bg, *fg, fg_on, *gains, *biases,
                                       img_lut.data_ptr(), gt_lut.data_ptr(), image.data_ptr(), gt.data_ptr(), 0, None)

    for which in ("bg", "fg"):
        for coeff in ((nan, 0.0, 0.0, 0.0, 1.0, 0.0), (1.0, 0.0, inf, 0.0, 1.0, 0.0), (1.0, 0.0, 0.0, 0.0, -inf, 0.0)):
            assert entry(**{which: coeff}) == E_ARG and b"non-finite coefficient" in Lib.fosvos_last_error()
        for coeff in ((1.0, 0.0, 2.0 ** 30 + 1, 0.0, 1.0, 0.0), (1.0, 0.0, 0.0, 0.0, 1.0, -(2.0 ** 30) - 1),
                      (2.0 ** 30, 0.0, 0.0, 0.0, 1.0, 0.0), (1e300, 0.0, 0.0, 0.0, 1.0, 0.0)):
            assert entry(**{which: coeff}) == E_ARG and b"beyond +-2^30" in Lib.fosvos_last_error(), (which, coeff)
    for kw in (dict(gains=(nan, 1.0, 1.0)), dict(gains=(1.0, 1.0, inf)), dict(biases=(0.0, -inf, 0.0)), dict(biases=(0.0, 0.0, nan))):
        assert entry(**kw) == E_ARG and b"non-finite gain or bias" in Lib.fosvos_last_error()
    for H, W in ((h, 8193), (8193, w), (0, w), (h, -1)):  # (checked before anything is read)
        assert entry(H=H, W=W) == E_SHAPE and b"<= 8192" in Lib.fosvos_last_error()
    assert entry(frame_ptr=None) == E_ARG and b"null pointer" in Lib.fosvos_last_error()
    torch.cuda.synchronize()
    image.fill_(float("nan"))
    assert entry(fg=(nan,) * 6, fg_on=0) == 0       # no object: its matrix is not looked at
    assert entry(bg=(1.0, 0.0, 2.0 ** 30 - w, 0.0, 1.0, -(2.0 ** 30))) == 0  # at the bound: taken (and all zeros)
    torch.cuda.synchronize()
    assert not image.any() and not gt.any()


# ------------------------------------------------------------------------------------------ the loader on the device
@pytest.fixture(scope="module")
def davis_root(tmp_path_factory):
    return write_davis_tree(tmp_path_factory.mktemp("davis_lucid_gpu"), seqs=SEQS, train=["bear"])


def test_device_loader_is_the_cpu_loader_draw_for_draw(davis_root):
    from dataloaders.resident import ResidentOneShotLoader
    from util import io_helper
    opts = LucidOptions()
    host = ResidentOneShotLoader(DAVIS2016(mode="train", db_root_dir=str(davis_root), seq_name="bear"), device=torch.device("cpu"),
                                 lucid=opts)
    dev = io_helper.get_data_loader_train(str(davis_root), 1, "bear", lucid=opts)
    assert isinstance(dev, ResidentOneShotLoader) and dev.device.type == "cuda"
    for t in (dev._frame, dev._background, dev._mask):
        assert t.is_cuda and t.dtype == torch.uint8
    assert torch.equal(dev._background.cpu(), torch.from_numpy(host._host[1])) and not torch.equal(dev._background, dev._frame)
    (ea, ra), (eb, rb) = lucid_epochs(host, 31), lucid_epochs(dev, 31)
    assert torch.equal(ra, rb) and len(ea) == len(eb) == N_EPOCHS and host.draws == dev.draws and len(dev.draws) == N_EPOCHS
    for xa, xb in zip(ea, eb):
        assert len(xa) == len(xb) == 1
        assert (xa[0]["seq_name"], xa[0]["fname"]) == (xb[0]["seq_name"], xb[0]["fname"])
        for key in ("image", "gt"):
            assert xb[0][key].is_cuda and xa[0][key].dtype == xb[0][key].dtype and xa[0][key].shape == xb[0][key].shape, key
            assert torch.equal(xa[0][key].view(torch.int32), xb[0][key].cpu().view(torch.int32)), key
    assert len({m[0]["image"].numpy().tobytes() for m in ea}) == N_EPOCHS
    assert torch.equal(dev.variants[(False, 0)]["image"].cpu(), host.variants[(False, 0)]["image"])


# ------------------------------------------------------------------------------------------ the loop
class _Writer:
    def add_scalar(self, *a, **k):
        pass

    def close(self):
        pass


def test_online_training_fed_by_the_loader_one_launch_a_draw(tmp_path, monkeypatch):
    """train_online._train for two epochs of the one 80 x 120 sample, a step every epoch, fed by the lucid loader: exactly one
    fosvos_lucid_sample call per draw, finite losses, and weights that moved."""
    import train_online
    from fosvos_hip import lib, ops
    from networks.osvos_vgg import OSVOS_VGG
    from oracle import osvos_ref as O
    from util import io_helper
    from util.network_provider import VGGOnlineProvider
    root = write_davis_tree(tmp_path, seqs={"a": (2, 80, 120)}, train=["a"])
    net = OSVOS_VGG(pretrained=0)
    net.load_state_dict(O.make_state_dict(6))
    prov = VGGOnlineProvider.__new__(VGGOnlineProvider)
    prov.name = "vgg16"
    prov.network = net.to(DEV)
    prov.save_model = lambda *a, **k: None
    opt = prov.get_optimizer(learning_rate=1e-6)
    torch.manual_seed(2024)
    loader = io_helper.get_data_loader_train(str(root), 1, "a", lucid=LucidOptions())
    counting = _Counting(lib())
    monkeypatch.setattr(ops, "lib", lambda: counting)
    monkeypatch.setattr(train_online, "data_parallel", False)
    ret = train_online._train(prov, loader, opt, _Writer(), "a", 0, 2, 1, 10 ** 9)
    torch.cuda.synchronize()
    assert ret["iterations"] == 2 and len(loader.draws) == 2 and counting.launches == 2
    assert len({d[1] for d in loader.draws}) == 2 and all(np.isfinite(v) for v in ret["loss"])
    init = O.make_state_dict(6)
    after = {k: v.detach().cpu() for k, v in prov.network.state_dict().items()}
    assert max((after[k] - init[k]).abs().max().item() for k in after) > 0  # the weights did train
