"""Rotating and zooming the training sample (ScaleNRotate in place of Resize) without a GPU: the numpy definition's
properties, the recipe of one thread of the HIP kernel (fosvos_warp_sample) written out on the host against that definition,
the resident loaders on the CPU device against the per-iteration DataLoader draw for draw, RotateOptions and the flags.
Every comparison is exact equality of bits."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))

from dataloaders import custom_transforms as T  # noqa: E402
from dataloaders.davis_2016 import DAVIS2016, MEANVAL  # noqa: E402
from fosvos_hip import limits  # noqa: E402
from fosvos_hip.options import RotateOptions  # noqa: E402
from test_resident_set_cpu import N_EPOCHS, _epochs, assert_same_epochs, write_davis_tree  # noqa: E402

# the matrices of the kernel tests: (degrees, zoom)
ROTATIONS = ((30.0, 0.75), (-30.0, 1.25), (90.0, 1.0), (12.34, 0.9))
SIZES = ((13, 17), (33, 130))
# five training sequences of four frame sizes (assert_same_epochs wants four shapes, and a warp keeps the source's), one of
# them with a mask of 0 / 7; one validation sequence
SEQS = {"bear": (3, 24, 40), "camel": (2, 24, 40), "cows": (2, 19, 33), "dog": (2, 21, 37), "elk": (1, 26, 35),
        "fox": (2, 24, 40)}
TRAIN = ["bear", "camel", "cows", "dog", "elk"]
FORMS = {"tuple": RotateOptions(), "list": RotateOptions(rots=[-30, 0, 30.5], scales=[0.75, 1, 1.25], renormalize=True)}


def _dataset():
    ds = DAVIS2016.__new__(DAVIS2016)
    ds.meanval = MEANVAL
    return ds


def sample_bytes(h, w, peak=255):
    rng = np.random.RandomState(h * 1000 + w)
    img = rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    lab = np.where(rng.rand(h, w) > 0.5, peak, 0).astype(np.uint8)
    lab[h // 3:, : w // 2] = peak // 2
    lab[0, 0] = peak
    return img, lab


def todays_class(sample, rot, sc):
    """ScaleNRotate.__call__ as the reference has it, with the draws fixed: the warp, then the two renormalisation steps."""
    out = {}
    for key, tmp in sample.items():
        h, w = tmp.shape[:2]
        tmp = T.warp_affine(tmp, T.rotation_matrix((w / 2, h / 2), rot, sc))
        if tmp.min() < 0.0:
            tmp = tmp - tmp.min()
        if tmp.max() > 1.0:
            tmp = tmp / tmp.max()
        out[key] = tmp
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------ 1. the definition
def test_definition_properties():
    ds = _dataset()
    image, gt = ds.convert_raw(*sample_bytes(24, 40))
    # rotation 0 at zoom 1 returns the sample exactly
    same = T.ScaleNRotate(rots=[0], scales=[1], renormalize=False)({"image": image.copy(), "gt": gt.copy(), "fname": "x"})
    assert np.array_equal(bits(same["image"]), bits(image)) and np.array_equal(bits(same["gt"]), bits(gt))
    assert same["fname"] == "x"
    # a translation by 1000 pixels leaves nothing of the source
    far = np.array([[1.0, 0.0, 1000.0], [0.0, 1.0, 1000.0]])
    assert not T.warp_affine(image, far).any() and not T.warp_affine(gt, far).any()
    assert T.warp_affine(image, far).dtype == np.float32 and T.warp_affine(gt, far).shape == gt.shape
    # renormalize=True (the default) is the class as the reference has it; False skips both steps
    assert T.ScaleNRotate().renormalize is True
    for rot, sc in ROTATIONS:
        want = todays_class({"image": image, "gt": gt}, rot, sc)
        got = T.ScaleNRotate(rots=[rot], scales=[sc])({"image": image.copy(), "gt": gt.copy()})
        plain = T.ScaleNRotate(rots=[rot], scales=[sc], renormalize=False)({"image": image.copy(), "gt": gt.copy()})
        m = T.rotation_matrix((40 / 2, 24 / 2), rot, sc)
        for key in ("image", "gt"):
            assert np.array_equal(bits(got[key]), bits(want[key])), (key, rot, sc)
            assert np.array_equal(bits(plain[key]), bits(T.warp_affine({"image": image, "gt": gt}[key], m))), (key, rot, sc)
        assert got["image"].min() == 0.0 and got["image"].max() == 1.0   # what the renormalisation is for
        assert plain["image"].min() < 0.0 and plain["image"].max() > 1.0
        assert np.array_equal(bits(got["gt"]), bits(plain["gt"]))        # on a mask it is a no-op


def test_draw_order_of_the_two_forms():
    import random

    class Rng:
        def __init__(self):
            self.calls = []

        def random(self):
            self.calls.append("random")
            return 0.75

        def randint(self, a, b):
            self.calls.append(("randint", a, b))
            return b

    r = Rng()
    assert T.ScaleNRotate((-30, 30), (.75, 1.25)).draw(r) == (60 * 0.75 - 30, 0.5 * 0.75 - 0.25 + 1)
    assert r.calls == ["random", "random"]
    r = Rng()
    assert T.ScaleNRotate([1, 2, 3], [4, 5]).draw(r) == (3, 5) and r.calls == [("randint", 0, 2), ("randint", 0, 1)]
    # __call__ draws from the module's ``random`` exactly what draw() draws
    image = np.zeros((6, 8, 3), np.float32)
    random.seed(5)
    rot, sc = T.ScaleNRotate().draw()
    random.seed(5)
    got = T.ScaleNRotate(renormalize=False)({"image": image + 1})
    assert np.array_equal(bits(got["image"]), bits(T.warp_affine(image + 1, T.rotation_matrix((4, 3), rot, sc))))


# ------------------------------------------------------------------------------------------ 2. the kernel's recipe
def f32(v):
    return np.float32(v)


def thread_cubic_weights(x):
    """cubic_weights of csrc/warp.hip: one fraction (here: every thread's, side by side), fp32, every operation rounded."""
    assert x.dtype == np.float32
    a = f32(-0.75)
    t = x + f32(1.0)
    w0 = ((a * t - f32(5.0) * a) * t + f32(8.0) * a) * t - f32(4.0) * a
    w1 = ((a + f32(2.0)) * x - (a + f32(3.0))) * x * x + f32(1.0)
    u = f32(1.0) - x
    w2 = ((a + f32(2.0)) * u - (a + f32(3.0))) * u * u + f32(1.0)
    w3 = f32(1.0) - w0 - w1 - w2
    for w in (w0, w1, w2, w3):
        assert w.dtype == np.float32
    return (w0, w1, w2, w3)


def emulate_kernel(ds, img_u8, lab_u8, flip, matrix, renormalize=False):
    """What one thread of k_warp does for its pixel (x, y), stated for all threads side by side: the six doubles of the
    inverse, the fp64 coordinates, int32 taps, the value tables, the clamped loads with the value replaced by 0 outside,
    fp32 products rounded before their adds; then the second launch's renormalisation from (min, max)."""
    h, w = lab_u8.shape
    ramp = np.repeat(np.arange(256, dtype=np.uint8)[:, None, None], 3, axis=2)
    img_lut = ds.convert_raw(ramp, None)[0].reshape(256, 3)
    gt_lut = np.arange(256, dtype=np.float32) / np.float32(max(float(lab_u8.max()), 1e-8))
    inv = np.linalg.inv(np.vstack([np.asarray(matrix, dtype=np.float64), [0.0, 0.0, 1.0]]))
    i00, i01, i02, i10, i11, i12 = (float(v) for v in inv[:2].reshape(-1))
    y, x = np.meshgrid(np.arange(h, dtype=np.int32), np.arange(w, dtype=np.int32), indexing="ij")
    xd, yd = x.astype(np.float64), y.astype(np.float64)
    sx = (i00 * xd + i01 * yd) + i02
    sy = (i10 * xd + i11 * yd) + i12
    assert np.abs(sx).max() <= 2 ** 30 and np.abs(sy).max() <= 2 ** 30
    mirror = (lambda c: w - 1 - c) if flip else (lambda c: c)
    # the mask
    xi, yi = np.rint(sx).astype(np.int32), np.rint(sy).astype(np.int32)
    inside = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
    gt = np.where(inside, gt_lut[lab_u8[np.clip(yi, 0, h - 1), mirror(np.clip(xi, 0, w - 1))]], f32(0.0))
    # the frame
    fx, fy = np.floor(sx), np.floor(sy)
    bx, by = fx.astype(np.int32), fy.astype(np.int32)
    wx, wy = thread_cubic_weights((sx - fx).astype(np.float32)), thread_cubic_weights((sy - fy).astype(np.float32))
    acc = np.zeros((h, w, 3), dtype=np.float32)
    chans = np.arange(3)[None, None, :]
    for j in range(4):
        yy = by + np.int32(j - 1)
        row_in = (yy >= 0) & (yy < h)
        yc = np.minimum(np.maximum(yy, 0), h - 1)
        for i in range(4):
            xx = bx + np.int32(i - 1)
            tap_in = row_in & (xx >= 0) & (xx < w)
            xc = mirror(np.minimum(np.maximum(xx, 0), w - 1))
            wgt = wy[j] * wx[i]
            val = np.where(tap_in[..., None], img_lut[img_u8[yc, xc], chans], f32(0.0))
            acc = acc + val * wgt[..., None]
    assert acc.dtype == np.float32 and gt.dtype == np.float32
    if renormalize:
        mn, mx = acc.min(), acc.max()
        shift = mn < 0.0
        mx2 = f32(mx - mn) if shift else mx
        div = mx2 > 1.0
        if shift:
            acc = acc - mn
        if div:
            acc = acc / mx2
        assert acc.dtype == np.float32
    return acc, gt


@pytest.mark.parametrize("size", SIZES)
def test_kernel_recipe_is_the_numpy_definition_bit_for_bit(size):
    h, w = size
    ds = _dataset()
    img, lab = sample_bytes(h, w)
    for rot, sc in ROTATIONS:
        matrix = T.rotation_matrix((w / 2, h / 2), rot, sc)
        for flip in (False, True):
            image, gt = ds.convert_raw(img, lab)
            if flip:
                image, gt = np.ascontiguousarray(image[:, ::-1]), np.ascontiguousarray(gt[:, ::-1])
            got_img, got_gt = emulate_kernel(ds, img, lab, flip, matrix)
            assert np.array_equal(bits(got_img), bits(T.warp_affine(image, matrix))), (size, rot, sc, flip)
            assert np.array_equal(bits(got_gt), bits(T.warp_affine(gt, matrix))), (size, rot, sc, flip)
            assert got_gt.any() and (got_gt == 0).any()
            # with the renormalisation: the class
            want = T.ScaleNRotate([rot], [sc], renormalize=True)({"image": image, "gt": gt})
            got_img, got_gt = emulate_kernel(ds, img, lab, flip, matrix, renormalize=True)
            assert np.array_equal(bits(got_img), bits(want["image"])), (size, rot, sc, flip)
            assert np.array_equal(bits(got_gt), bits(want["gt"])), (size, rot, sc, flip)


# ------------------------------------------------------------------------------------------ 3. the loaders replay
@pytest.fixture(scope="module")
def davis_root(tmp_path_factory):
    return write_davis_tree(tmp_path_factory.mktemp("davis_rotate"), seqs=SEQS, train=TRAIN)


def assert_same_one_shot_epochs(a, b):
    """assert_same_epochs for a one-sample loader: the same checks, tensor for tensor, without its demand for four shapes
    (a warp keeps the one frame's size)."""
    (ea, ra), (eb, rb) = a, b
    assert torch.equal(ra, rb) and len(ea) == len(eb) == N_EPOCHS
    for xa, xb in zip(ea, eb):
        assert len(xa) == len(xb) == 1
        assert (xa[0]["seq_name"], xa[0]["fname"]) == (xb[0]["seq_name"], xb[0]["fname"])
        for key in ("image", "gt"):
            assert xa[0][key].dtype == xb[0][key].dtype and tuple(xa[0][key].shape) == tuple(xb[0][key].shape), key
            assert torch.equal(xa[0][key].view(torch.int32), xb[0][key].cpu().view(torch.int32)), key
    assert len({m[0]["image"].numpy().tobytes() for m in ea}) > N_EPOCHS // 2  # the warps differ (a list has 18 outcomes)


@pytest.mark.parametrize("form", sorted(FORMS))
def test_cpu_one_shot_loader_replays_the_dataloader(davis_root, form):
    from torch.utils.data import DataLoader
    from util import io_helper
    from dataloaders.resident import ResidentOneShotLoader
    runs, loaders = [], []
    for resident in (False, True):
        torch.manual_seed(77)
        if resident:
            loader = ResidentOneShotLoader(DAVIS2016(mode="train", db_root_dir=str(davis_root), seq_name="bear"),
                                           device=torch.device("cpu"), rotate=FORMS[form])
        else:
            loader = io_helper.get_data_loader_train(str(davis_root), 1, "bear", resident=False, rotate=FORMS[form])
            assert type(loader) is DataLoader
        assert len(loader) == 1
        runs.append(_epochs(loader, N_EPOCHS))
        loaders.append(loader)
    assert_same_one_shot_epochs(*runs)
    draws = loaders[1].draws
    assert len(draws) == N_EPOCHS and all(len(d) == 3 and isinstance(d[0], bool) for d in draws)
    if form == "list":
        assert {d[1] for d in draws} <= {-30, 0, 30.5} and {d[2] for d in draws} <= {0.75, 1, 1.25}
    else:
        assert all(-30 <= d[1] <= 30 and 0.75 <= d[2] <= 1.25 for d in draws) and len({d[1:] for d in draws}) == N_EPOCHS
    # the factory hands the option to the resident loader too
    made = io_helper.get_data_loader_train(str(davis_root), 1, "bear", rotate=FORMS[form])
    assert isinstance(made, ResidentOneShotLoader) and made.rotate is FORMS[form]


@pytest.mark.parametrize("shard", [None, (0, 2), (1, 2)])
@pytest.mark.parametrize("form", sorted(FORMS))
def test_cpu_set_loader_replays_the_dataloader(davis_root, form, shard):
    from util import io_helper
    from dataloaders.resident import ResidentTrainSetLoader
    runs = []
    for resident_set in (False, True):
        torch.manual_seed(123)
        if resident_set:
            loader = ResidentTrainSetLoader(DAVIS2016(mode="train", db_root_dir=str(davis_root)), device="cpu", shard=shard,
                                            rotate=FORMS[form])
        else:
            loader = io_helper.get_data_loader_train(str(davis_root), 1, shard=shard, rotate=FORMS[form])
            assert not isinstance(loader, ResidentTrainSetLoader)
        assert len(loader) == (10 if shard is None else 5)
        runs.append(_epochs(loader, N_EPOCHS, set_epoch=shard is not None))
    assert_same_epochs(*runs)
    assert len(loader.draws) == N_EPOCHS * len(loader)
    # every sample keeps its own size
    sizes = {tuple(m["image"].shape[2:]) for ep in runs[1][0] for m in ep}
    assert sizes == {(24, 40), (19, 33), (21, 37), (26, 35)}


def test_factory_refuses_rotation_of_the_synthetic_sequence(davis_root):
    from util import io_helper
    with pytest.raises(ValueError, match="synthetic loader augments nothing"):
        io_helper.get_data_loader_train(str(davis_root), 1, synthetic=(24, 40), rotate=RotateOptions())
    # without the option the factory makes what it made
    from dataloaders.resident import ResidentOneShotLoader
    plain = io_helper.get_data_loader_train(str(davis_root), 1, "bear")
    assert isinstance(plain, ResidentOneShotLoader) and plain.rotate is None and len(plain.variants) == 6
    assert plain.scales == [0.5, 0.8, 1]


# ------------------------------------------------------------------------------------------ 4. the unaugmented frame
def test_first_sample_of_a_rotating_loader_is_the_unaugmented_frame(davis_root):
    import train_online
    from dataloaders.resident import ResidentOneShotLoader
    ds = DAVIS2016(mode="train", db_root_dir=str(davis_root), seq_name="camel")
    loader = ResidentOneShotLoader(ds, device=torch.device("cpu"), rotate=RotateOptions(renormalize=True))
    list(loader)
    first = train_online._first_sample(loader)
    want = T.ToTensor()(dict(zip(("image", "gt"), ds.make_img_gt_pair(0))))
    assert set(first) == {"image", "gt"}
    assert torch.equal(first["image"], want["image"][None]) and torch.equal(first["gt"], want["gt"][None])
    assert loader.scales == [1] and list(loader.variants) == [(False, 0)]
    # ... which is what the loader without rotation hands out
    plain = train_online._first_sample(ResidentOneShotLoader(ds, device=torch.device("cpu")))
    assert torch.equal(first["image"], plain["image"]) and torch.equal(first["gt"], plain["gt"])
    assert np.array_equal(train_online._train_annotation(loader), (want["gt"][0].numpy() >= 0.5).astype(np.uint8))


# ------------------------------------------------------------------------------------------ 5. RotateOptions
def test_rotate_options_validation():
    d = RotateOptions()
    assert d.rots == (-30.0, 30.0) and d.scales == (0.75, 1.25) and d.renormalize is False
    with pytest.raises(Exception):
        d.renormalize = True  # frozen
    assert limits.ROTATE_MAX_ANGLE == 360.0 and limits.ROTATE_SCALE_RANGE == (1 / 16, 16.0)
    good = [dict(rots=(-360, 360), scales=(1.0, 1.0)), dict(rots=(0, 0), scales=(1 / 16, 1.9375)),
            dict(rots=[360], scales=[16]), dict(rots=[-360.0, 12.5], scales=[1 / 16]), dict(renormalize=True)]
    for kw in good:
        t = RotateOptions(**kw).transform()
        assert isinstance(t, T.ScaleNRotate) and t.renormalize is kw.get("renormalize", False)
    assert RotateOptions(rots=[1, 2], scales=[3]).transform().rots == [1, 2]
    bad = [dict(rots=(-30, 30), scales=[0.75, 1.25]), dict(rots=[-30, 30]), dict(rots=30, scales=1), dict(rots=None, scales=None),
           dict(rots=(-361, 0)), dict(rots=(0, float("nan"))), dict(rots=[float("inf")], scales=[1]), dict(rots=[True], scales=[1]),
           dict(scales=(0.05, 1)), dict(scales=(1, 16.5)), dict(rots=[0], scales=[0]), dict(rots=[0], scales=["1"]),
           dict(rots=(1, 2, 3)), dict(scales=(1,)), dict(rots=[], scales=[]), dict(rots=(30, -30)), dict(scales=(1.25, 0.75)),
           dict(scales=(1 / 16, 2.0)),  # the draw 1 +- (hi - lo) / 2 would reach below 1/16
           dict(renormalize=1), dict(renormalize=None)]
    for kw in bad:
        with pytest.raises(ValueError, match="^RotateOptions: "):
            RotateOptions(**kw)
    with pytest.raises(ValueError) as e:
        RotateOptions(rots=(-400, 0))
    assert str(e.value) == "RotateOptions: rots must be a finite number in [-360, 360], got -400"
    with pytest.raises(ValueError) as e:
        RotateOptions(scales=(0.01, 1))
    assert str(e.value) == "RotateOptions: scales must be a finite number in [0.0625, 16], got 0.01"


# ------------------------------------------------------------------------------------------ 6. the flags
@pytest.mark.parametrize("is_online", [True, False])
def test_flags_parse(is_online):
    from util import args_helper
    assert args_helper.parse_args(is_online=is_online, argv=[]).rotate is None
    assert args_helper.parse_args(is_online=is_online, argv=["--augment-rotate"]).rotate == RotateOptions()
    got = args_helper.parse_args(is_online=is_online, argv=["--augment-rotate", "--rotate-range", "-10", "20.5", "--zoom-range",
                                                            "0.9", "1.5", "--rotate-renormalize"]).rotate
    assert got == RotateOptions(rots=(-10.0, 20.5), scales=(0.9, 1.5), renormalize=True)
    for argv in (["--rotate-range", "-10", "10"], ["--zoom-range", "0.9", "1.1"], ["--rotate-renormalize"],
                 ["--augment-rotate", "--synthetic"], ["--augment-rotate", "--data-parallel"],
                 ["--augment-rotate", "--rotate-range", "10", "-10"], ["--augment-rotate", "--rotate-range", "-400", "0"],
                 ["--augment-rotate", "--zoom-range", "0.01", "1"], ["--augment-rotate", "--rotate-range", "5"]):
        with pytest.raises(SystemExit):
            args_helper.parse_args(is_online=is_online, argv=argv)


def test_flag_refusals_give_the_reason(capsys):
    from util import args_helper
    for argv, reason in ((["--zoom-range", "0.9", "1.1"], "--zoom-range set(s) an option of the rotation: it needs --augment-rotate"),
                         (["--rotate-range", "1", "2", "--rotate-renormalize"], "--rotate-range / --rotate-renormalize set(s)"),
                         (["--augment-rotate", "--synthetic"], "the loader of --synthetic augments nothing"),
                         (["--augment-rotate", "--data-parallel"], "not wired to the sharded loaders of --data-parallel"),
                         (["--augment-rotate", "--rotate-range", "-400", "0"], "--augment-rotate: rots must be a finite number")):
        with pytest.raises(SystemExit):
            args_helper.parse_args(is_online=True, argv=argv)
        assert reason in capsys.readouterr().err, argv


def test_online_flag_combines_with_the_other_passes():
    from util import args_helper
    for extra in (["--multi-object"], ["--adapt-steps", "1"], ["--score"], ["--fast-test"], ["--fast-test", "--score", "--png-fitted"],
                  ["--fast-test", "--clean-largest"], ["--device-decode"]):
        assert args_helper.parse_args(is_online=True, argv=["--augment-rotate"] + extra).rotate == RotateOptions()
    for extra in (["--resident-train-set"], ["--microbatch-group", "5"], ["--resident-train-set", "--microbatch-group", "5"]):
        assert args_helper.parse_args(is_online=False, argv=["--augment-rotate"] + extra).rotate == RotateOptions()


def test_offline_main_passes_the_option(monkeypatch, tmp_path):
    import train_offline
    from util import io_helper
    seen = {}

    def fake_loader(*args, **kwargs):
        seen["kwargs"] = kwargs
        raise KeyboardInterrupt  # (far enough)

    monkeypatch.setattr(train_offline.gpu_handler, "select_gpu", lambda *a, **k: None)
    monkeypatch.setattr(train_offline, "rotate", None)
    monkeypatch.setattr(train_offline, "resident_train_set", False)
    monkeypatch.setattr(train_offline, "save_dir_models", tmp_path / "models")
    monkeypatch.setattr(train_offline, "save_dir_results", tmp_path / "results")
    monkeypatch.setattr(train_offline.io_helper, "get_data_loader_train", fake_loader)
    monkeypatch.setattr(train_offline.io_helper, "write_settings", lambda *a, **k: None)
    monkeypatch.setattr(train_offline.provider_mapping[("offline", "vgg16")], "load_network_train", lambda self: None)
    assert io_helper is train_offline.io_helper
    with pytest.raises(KeyboardInterrupt):
        train_offline.main(["--augment-rotate", "--zoom-range", "0.9", "1.1", "--resident-train-set", "--no-testing"])
    assert seen["kwargs"]["rotate"] == RotateOptions(scales=(0.9, 1.1)) and seen["kwargs"]["resident_set"] is True
    assert train_offline.rotate == RotateOptions(scales=(0.9, 1.1))
    with pytest.raises(KeyboardInterrupt):
        train_offline.main(["--no-testing"])
    assert "rotate" not in seen["kwargs"] and train_offline.rotate is None  # absent: the call is what it was


def test_online_main_passes_the_option(monkeypatch, tmp_path):
    import train_online
    seen = []

    def fake_loader(*args, **kwargs):
        seen.append(("sequence", args[2], kwargs))
        raise KeyboardInterrupt

    class FakeOneShot:
        def __init__(self, dataset, **kwargs):
            seen.append(("object", dataset, kwargs))
            raise KeyboardInterrupt

    monkeypatch.setattr(train_online.gpu_handler, "select_gpu", lambda *a, **k: None)
    monkeypatch.setattr(train_online, "rotate", None)
    monkeypatch.setattr(train_online, "save_dir_models", tmp_path / "models")
    monkeypatch.setattr(train_online, "save_dir_results", tmp_path / "results")
    monkeypatch.setattr(train_online.io_helper, "get_data_loader_train", fake_loader)
    monkeypatch.setattr(train_online.io_helper, "write_settings", lambda *a, **k: None)
    monkeypatch.setattr(train_online.provider_mapping[("online", "vgg16")], "load_network_train", lambda self: None)
    with pytest.raises(KeyboardInterrupt):
        train_online.main(["--augment-rotate", "--rotate-renormalize", "-s", "bear", "--no-testing"])
    assert seen[-1] == ("sequence", "bear", {"synthetic": None, "rotate": RotateOptions(renormalize=True)})
    with pytest.raises(KeyboardInterrupt):
        train_online.main(["-s", "bear", "--no-testing"])
    assert seen[-1] == ("sequence", "bear", {"synthetic": None}) and train_online.rotate is None
    # the per-object loaders of --multi-object
    import dataloaders.davis_2017 as D17
    import dataloaders.resident as R
    monkeypatch.setattr(D17, "n_objects", lambda root, seq: 2)
    monkeypatch.setattr(D17, "DAVIS2017", lambda **kw: ("dataset", kw["seq_name"], kw["object_id"]))
    monkeypatch.setattr(R, "ResidentOneShotLoader", FakeOneShot)
    monkeypatch.setattr(train_online, "_get_summary_writer", lambda *a, **k: None)
    with pytest.raises(KeyboardInterrupt):
        train_online.main(["--augment-rotate", "--multi-object", "-s", "bear", "--no-testing"])
    assert seen[-1] == ("object", ("dataset", "bear", 1), {"rotate": RotateOptions()})
    with pytest.raises(KeyboardInterrupt):
        train_online.main(["--multi-object", "-s", "bear", "--no-testing"])
    assert seen[-1] == ("object", ("dataset", "bear", 1), {})
