"""Online adaptation, host side: the numpy definitions (util/online_adapt.py) against a brute force, scipy and the oracle's
loss; AdaptOptions; the flag combinations train_online accepts and refuses; ``test_adaptive`` on a CPU stand-in net; and the
argument checks of the C entries, which answer with error codes before any device is touched.  No GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import online_adapt_cases as C  # noqa: E402
from oracle import osvos_ref as O  # noqa: E402
from util import online_adapt as A  # noqa: E402

GATE_CASES = list(C.gate_cases())


# ------------------------------------------------------------------------------------------ far_from
def test_far_from_equals_the_brute_force():
    n = 0
    for name, mask, d in GATE_CASES:
        if mask.shape not in C.BRUTE_SHAPES:
            continue
        for invert in (False, True):
            assert np.array_equal(A.far_from(mask, d, invert), C.brute_far_from(mask, d, invert)), (name, invert)
            n += 1
    assert n >= 2 * 3 * 6 * 6


def test_far_from_equals_scipys_transform_and_erosion():
    ndimage = pytest.importorskip("scipy.ndimage")
    for name, mask, d in GATE_CASES:
        for invert in (False, True):
            s = (mask != 0) != invert
            got = A.far_from(mask, d, invert)
            assert got.dtype == np.uint8 and got.shape == mask.shape
            if not s.any():
                assert got.all(), (name, invert)
                continue
            # the nearest set pixel's index from scipy, the squared distance to it in integers
            idx = ndimage.distance_transform_edt(~s, return_distances=False, return_indices=True)
            y, x = np.mgrid[0:mask.shape[0], 0:mask.shape[1]]
            d2 = (idx[0].astype(np.int64) - y) ** 2 + (idx[1].astype(np.int64) - x) ** 2
            assert np.array_equal(got, (d2 > d * d).astype(np.uint8)), (name, invert)
    for h, w in C.SHAPES:
        for e in (1, 2, 4):
            yy, xx = np.mgrid[-e:e + 1, -e:e + 1]
            disk = (yy * yy + xx * xx) <= e * e
            for name, mask in C.masks(h, w, e).items():
                want = ndimage.binary_erosion(mask != 0, disk, border_value=1)
                assert np.array_equal(A.far_from(mask, e, invert=True), want.astype(np.uint8)), (h, w, e, name)


def test_far_from_counts_equality_as_near():
    m = np.zeros((40, 52), np.uint8)
    m[10, 10] = 1
    for k in (1, 2, 6):
        assert A.far_from(m, 5 * k)[10 + 3 * k, 10 + 4 * k] == 0      # exactly 5k away: not further
        assert A.far_from(m, 5 * k - 1)[10 + 3 * k, 10 + 4 * k] == 1
    assert A.far_from(m, 0)[10, 10] == 0 and A.far_from(m, 0).sum() == m.size - 1
    assert A.far_from(np.zeros((3, 5), np.uint8), 0).all()            # no set pixel: vacuously far
    assert not A.far_from(np.zeros((3, 5), np.uint8), 0, invert=True).any()
    for bad in (lambda: A.far_from(m, -1), lambda: A.far_from(m, 4096), lambda: A.far_from(m, 2.0),
                lambda: A.far_from(m, True), lambda: A.far_from(m.astype(np.float32), 1), lambda: A.far_from(m[0], 1)):
        with pytest.raises(ValueError):
            bad()


# ------------------------------------------------------------------------------------------ adapt_labels
def test_adapt_labels_rules():
    for name, x, m, t, d, e in C.label_cases():
        label, void, counts = A.adapt_labels(x, m, t, d, e)
        assert label.dtype == np.float32 and void.dtype == np.uint8 and counts.sum() == x.size, name
        core = A.far_from(m, e, invert=True) if e > 0 else (m != 0).astype(np.uint8)
        far = C.brute_far_from(core, d).astype(bool) if core.any() else np.zeros(x.shape, bool)
        with np.errstate(invalid="ignore"):
            confident = x >= np.float32(t)
        assert np.array_equal(label == 1, ~far & confident), name          # far beats confident
        assert np.array_equal(void == 1, ~far & ~confident), name
        assert not np.any(label[far]) and not np.any(void[far]), name
        assert counts.tolist() == [int((~far & confident).sum()), int(far.sum()), int((~far & ~confident).sum())], name
        if not core.any():
            assert counts[1] == 0, name                                    # an empty core names no negatives


def test_adapt_labels_special_values():
    cases = {name: rest for name, *rest in C.label_cases()}
    x, m, t, d, e = cases["specials_near"]
    label, void, counts = A.adapt_labels(x, m, t, d, e)
    assert counts[1] == 0
    #            nan inf -inf -0 +0 | t  below above 100 -100 | nan inf t  t  7
    assert label.astype(int).tolist() == [[0, 1, 0, 0, 0], [1, 0, 1, 1, 0], [0, 1, 1, 1, 1]]
    assert void.tolist() == [[1, 0, 1, 1, 1], [0, 1, 0, 0, 1], [1, 0, 0, 0, 0]]
    x, m, t, d, e = cases["specials_far"]
    label, void, counts = A.adapt_labels(x, m, t, d, e)
    far = C.brute_far_from(m, d).astype(bool)
    assert far[0, 3] and far[2, 4] and not far[0, 1]
    assert not label[far].any() and not void[far].any()                    # +inf and a confident 7.0 far away: negatives
    assert label[0, 1] == 1 and void[0, 0] == 1
    with pytest.raises(ValueError):
        A.adapt_labels(x, m, float("nan"), 1, 0)
    with pytest.raises(ValueError):
        A.adapt_labels(x.astype(np.float64), m, 1.0, 1, 0)
    with pytest.raises(ValueError):
        A.adapt_labels(x, m[:2], 1.0, 1, 0)


def test_net_like_case_fills_every_class():
    h, w = C.NET_LIKE["shape"]
    x, m = C.logits_for(h, w)
    _, _, counts = A.adapt_labels(x, m, C.pos_logit(C.NET_LIKE["pos_prob"]), C.NET_LIKE["neg_distance"], C.NET_LIKE["erode"])
    share = counts / float(h * w)
    print("net-like case: positives %.1f %%, negatives %.1f %%, void %.1f %%" % tuple(100 * share))
    assert counts.sum() == h * w and (share >= 0.05).all(), share


# ------------------------------------------------------------------------------------------ cbce_void
@pytest.mark.parametrize("size_average", [False, True])
def test_cbce_void_without_void_is_the_oracles_loss(size_average):
    for n, h, w in ((1, 3, 5), (2, 40, 52), (3, 48, 86)):
        x, y, _ = C.loss_inputs(n, h, w)
        for k in range(n):
            xt, yt = torch.from_numpy(x[k:k + 1]).double(), torch.from_numpy(y[k:k + 1]).double()
            want = float(O.cbce_loss(xt, yt, size_average))
            want_g = O.cbce_loss_grad(xt, yt, size_average).numpy()
            loss, grad = A.cbce_void(x[k:k + 1], y[k:k + 1], np.zeros_like(y[k:k + 1], dtype=np.uint8), size_average)
            assert abs(loss - want) <= 1e-12 * max(1.0, abs(want))
            assert np.abs(grad - want_g).max() <= 1e-12
            # the torch statement of the same loss, and its autograd gradient
            leaf = xt.clone().requires_grad_(True)
            tl = A.cbce_void_torch(leaf, yt, None, size_average)
            tl.backward()
            assert abs(float(tl.detach()) - want) <= 1e-12 * max(1.0, abs(want)) and np.abs(leaf.grad.numpy() - want_g).max() <= 1e-12


def test_cbce_void_ignores_void_pixels():
    x, y, v = C.loss_inputs(1, 40, 52)
    loss, grad = A.cbce_void(x, y, v, False)
    valid = v == 0
    # the loss of the valid pixels alone, as a smaller tensor without void
    want, want_g = A.cbce_void(x[valid], y[valid], np.zeros(int(valid.sum()), np.uint8), False)
    assert abs(loss - want) <= 1e-12 * abs(want) and np.abs(grad[valid] - want_g).max() <= 1e-12
    assert not grad[~valid].any() and not np.signbit(grad[~valid]).any()
    poisoned = x.copy()
    poisoned[~valid] = np.nan
    loss2, grad2 = A.cbce_void(poisoned, y, v, False)
    assert loss2 == loss and np.array_equal(grad2, grad)
    loss0, grad0 = A.cbce_void(x, y, np.ones_like(v), True)
    assert loss0 == 0.0 and not grad0.any()
    leaf = torch.from_numpy(poisoned).double().requires_grad_(True)
    tl = A.cbce_void_torch(leaf, torch.from_numpy(y), torch.from_numpy(v), False)
    tl.backward()
    assert abs(float(tl.detach()) - loss) <= 1e-9 * abs(loss) and np.abs(leaf.grad.numpy() - grad).max() <= 1e-9
    assert "void_pixels" in A.cbce_void.__doc__ and "NOT" in A.cbce_void.__doc__


# ------------------------------------------------------------------------------------------ options, flags
def test_adapt_options_validation():
    import dataclasses
    import math
    from fosvos_hip.options import AdaptOptions
    o = AdaptOptions()
    assert (o.steps, o.pos_prob, o.neg_distance, o.erode, o.frame_weight, o.first_weight) == (1, 0.97, 220, 15, 1.0, 1.0)
    assert o.pos_logit == float(np.float32(math.log(0.97 / 0.03))) == C.pos_logit(0.97)
    assert o.as_dict() == {"steps": 1, "pos_prob": 0.97, "pos_logit": o.pos_logit, "neg_distance": 220, "erode": 15,
                           "frame_weight": 1.0, "first_weight": 1.0, "learning_rate": 1e-8}
    assert AdaptOptions(steps=0, first_weight=0, neg_distance=0, erode=4095).steps == 0
    with pytest.raises(dataclasses.FrozenInstanceError):
        o.steps = 2
    for bad in (dict(steps=-1), dict(steps=1.0), dict(steps=True), dict(pos_prob=0.5), dict(pos_prob=1.0), dict(pos_prob=float("nan")),
                dict(pos_prob="0.9"), dict(neg_distance=-1), dict(neg_distance=4096), dict(neg_distance=2.0), dict(erode=-1),
                dict(erode=4096), dict(erode=False), dict(frame_weight=0), dict(frame_weight=float("inf")), dict(first_weight=-0.1),
                dict(first_weight=None), dict(learning_rate=0), dict(learning_rate=-1e-8), dict(learning_rate=float("nan"))):
        with pytest.raises(ValueError, match="AdaptOptions"):
            AdaptOptions(**bad)


def test_train_online_adapt_flags():
    from util import args_helper
    a = args_helper.parse_args(True, ["--synthetic", "--adapt-steps", "2"])
    assert a.adapt.as_dict() == dict(steps=2, pos_prob=0.97, pos_logit=C.pos_logit(0.97), neg_distance=220, erode=15,
                                     frame_weight=1.0, first_weight=1.0, learning_rate=1e-8)
    a = args_helper.parse_args(True, ["--synthetic", "--adapt-steps", "1", "--adapt-pos-prob", "0.9", "--adapt-distance", "50",
                                      "--adapt-erode", "0", "--adapt-frame-weight", "0.5", "--adapt-first-weight", "0",
                                      "--adapt-lr", "1e-6", "--score", "--png-fitted"])
    assert (a.adapt.pos_prob, a.adapt.neg_distance, a.adapt.erode, a.adapt.frame_weight, a.adapt.first_weight,
            a.adapt.learning_rate) == (0.9, 50, 0, 0.5, 0.0, 1e-6)
    assert a.score and a.png_fitted
    assert args_helper.parse_args(True, ["--synthetic"]).adapt is None
    refused = [["--adapt-steps", "1", "--multi-object"], ["--adapt-steps", "1", "--data-parallel"],
               ["--adapt-steps", "1", "--eval-speeds"], ["--adapt-steps", "1", "--device-decode"],
               ["--adapt-steps", "1", "--fast-test", "--clean-min-area", "10"], ["--adapt-steps", "1", "--fast-test", "--clean-largest"],
               ["--adapt-steps", "1", "--fast-test", "--clean-temporal", "3"], ["--adapt-steps", "0"], ["--adapt-steps", "-2"],
               ["--adapt-pos-prob", "0.9"], ["--adapt-distance", "10"], ["--adapt-erode", "1"], ["--adapt-frame-weight", "1"],
               ["--adapt-first-weight", "1"], ["--adapt-lr", "1e-8"],
               ["--adapt-steps", "1", "--adapt-pos-prob", "0.4"], ["--adapt-steps", "1", "--adapt-distance", "5000"],
               ["--adapt-steps", "1", "--adapt-erode", "-1"], ["--adapt-steps", "1", "--adapt-frame-weight", "0"],
               ["--adapt-steps", "1", "--adapt-first-weight", "-1"], ["--adapt-steps", "1", "--adapt-lr", "0"]]
    for flags in refused:
        with pytest.raises(SystemExit):
            args_helper.parse_args(True, ["--synthetic"] + flags)
    with pytest.raises(SystemExit):
        args_helper.parse_args(False, ["--synthetic", "--adapt-steps", "1"])   # an online flag


def test_each_refusal_gives_its_reason(capsys):
    from util import args_helper
    for flags, word in ((["--adapt-steps", "1", "--multi-object"], "multi-object"),
                        (["--adapt-steps", "1", "--data-parallel"], "data-parallel"),
                        (["--adapt-steps", "1", "--eval-speeds"], "eval-speeds"),
                        (["--adapt-steps", "1", "--device-decode"], "device-decode"),
                        (["--adapt-steps", "1", "--fast-test", "--clean-largest"], "clean"),
                        (["--adapt-erode", "1"], "--adapt-steps")):
        with pytest.raises(SystemExit):
            args_helper.parse_args(True, ["--synthetic"] + flags)
        assert word in capsys.readouterr().err, flags


# ------------------------------------------------------------------------------------------ test_adaptive, host branch
class _Net(torch.nn.Module):
    """A one-layer stand-in that stays on the host: logits = a 3x3 conv of the frame's first channel."""

    def __init__(self, journal):
        super().__init__()
        self.conv = torch.nn.Conv2d(1, 1, 3, padding=1)
        with torch.no_grad():
            self.conv.weight.fill_(0.02)
            self.conv.bias.fill_(-1.0)
        self.journal = journal

    def forward(self, x):
        x = x.cpu()
        self.journal.append(("forward", torch.is_grad_enabled(), float(x.sum())))
        return [self.conv(x[:, :1])]


class _Sgd(torch.optim.SGD):
    def __init__(self, params, journal, **kw):
        super().__init__(params, **kw)
        self.journal = journal

    def zero_grad(self, set_to_none=True):
        self.journal.append(("zero_grad",))
        super().zero_grad(set_to_none=set_to_none)

    def step(self, closure=None):
        self.journal.append(("step",))
        return super().step(closure)


class _Provider:
    def __init__(self):
        self.journal, self.optimizers = [], []
        self.network = _Net(self.journal)

    def get_optimizer(self, learning_rate=1e-8):
        self.optimizers.append(_Sgd(self.network.parameters(), self.journal, lr=learning_rate))
        return self.optimizers[-1]


def _loaders(size=(24, 40), n_frames=3, batch=1):
    from util import io_helper
    loader = io_helper.get_data_loader_test(None, batch, "blob", synthetic=size, n_frames=n_frames)
    train = io_helper.get_data_loader_train(None, 1, "blob", synthetic=size)
    return loader, {"image": train.dataset[0]["image"], "gt": train.dataset[0]["gt"]}


def test_adaptive_host_branch_order_chain_and_trace(tmp_path):
    from fosvos_hip.options import AdaptOptions
    from util import experiment_helper
    loader, first = _loaders()
    prov = _Provider()
    adapt = AdaptOptions(steps=2, pos_prob=0.6, neg_distance=6, erode=1, frame_weight=0.5, first_weight=1.0, learning_rate=1e-4)
    trace = []
    before = [p.detach().clone() for p in prov.network.parameters()]
    score = experiment_helper.test_adaptive(prov, loader, tmp_path, first, adapt, loader.dataset.annotation, seq_name="blob",
                                            trace=trace)
    assert len(prov.optimizers) == 1 and prov.optimizers[0].param_groups[0]["lr"] == 1e-4
    first_sum = float(first["image"].sum())
    frames = [float(mb["image"].sum()) for mb in loader]
    want = []
    for s in frames:  # per frame: logits0, then per step zero / first frame / frame / step, then logits1
        want.append(("forward", False, s))
        for _ in range(2):
            want += [("zero_grad",), ("forward", True, first_sum), ("forward", True, s), ("step",)]
        want.append(("forward", False, s))
    assert prov.journal == want
    assert any(not torch.equal(a, b.detach()) for a, b in zip(before, prov.network.parameters()))   # the net leaves adapted
    # the chain: frame 0 starts from the annotation, frame t from frame t - 1's logits1 >= 0
    assert len(trace) == 3
    assert torch.equal(trace[0]["last_mask"][0], (first["gt"][0] >= 0.5).to(torch.uint8))
    for t in range(1, 3):
        assert torch.equal(trace[t]["last_mask"], (trace[t - 1]["logits1"][:, 0] >= 0).to(torch.uint8))
    for t, item in enumerate(trace):
        label, void, counts = A.adapt_labels(item["logits0"][0, 0].numpy(), item["last_mask"][0].numpy(), adapt.pos_logit, 6, 1)
        assert np.array_equal(item["label"][0, 0].numpy(), label) and np.array_equal(item["void"][0, 0].numpy(), void)
        assert score["adapt"]["counts"][t] == counts.tolist()
    assert score["adapt"]["steps"] == 2 and score == experiment_helper.last_score
    assert experiment_helper.last_fast["adapt"] == score["adapt"]
    assert sorted(p.name for p in (tmp_path / "blob").iterdir()) == ["%05d.png" % k for k in range(3)]


def test_adaptive_without_steps_writes_test_fasts_files(tmp_path):
    from fosvos_hip.options import AdaptOptions
    from util import experiment_helper
    loader, first = _loaders()
    prov = _Provider()
    fast = experiment_helper.test_fast(prov, loader, tmp_path / "fast", loader.dataset.annotation, seq_name="blob")
    n_fast = len(prov.journal)
    score = experiment_helper.test_adaptive(prov, loader, tmp_path / "adapt", first, AdaptOptions(steps=0),
                                            loader.dataset.annotation, seq_name="blob")
    assert not prov.optimizers                                              # no optimizer is constructed ...
    assert [j[:2] for j in prov.journal[n_fast:]] == [("forward", False)] * 3   # ... and nothing trains: one forward a frame
    names = sorted(p.name for p in (tmp_path / "fast" / "blob").iterdir())
    assert names == sorted(p.name for p in (tmp_path / "adapt" / "blob").iterdir()) and len(names) == 3
    for name in names:
        assert (tmp_path / "fast" / "blob" / name).read_bytes() == (tmp_path / "adapt" / "blob" / name).read_bytes()
    for key in ("counts", "J", "F", "fnames", "scored", "radius"):
        assert score[key] == fast[key]


def test_adaptive_refuses_batches_and_bad_arguments(tmp_path):
    from fosvos_hip.options import AdaptOptions, CleanOptions
    from util import experiment_helper
    loader2, first = _loaders(batch=2)
    with pytest.raises(ValueError, match="one at a time"):
        experiment_helper.test_adaptive(_Provider(), loader2, tmp_path, first, AdaptOptions(steps=0))
    loader, _ = _loaders()
    with pytest.raises(ValueError, match="AdaptOptions"):
        experiment_helper.test_adaptive(_Provider(), loader, tmp_path, first, CleanOptions())
    with pytest.raises(ValueError, match="png_huffman"):
        experiment_helper.test_adaptive(_Provider(), loader, tmp_path, first, AdaptOptions(), png_huffman="best")
    with pytest.raises(ValueError, match="first_sample"):
        experiment_helper.test_adaptive(_Provider(), loader, tmp_path, {"image": first["image"], "gt": first["gt"][:, :5]},
                                        AdaptOptions())
    other, _ = _loaders(size=(16, 24))
    with pytest.raises(ValueError, match="first_sample"):
        experiment_helper.test_adaptive(_Provider(), other, tmp_path, first, AdaptOptions(steps=0))


# ------------------------------------------------------------------------------------------ the C entries' checks
E_SHAPE, E_ARG, E_WORKSPACE = -1, -2, -3


def test_c_entries_refuse_bad_arguments_before_any_launch():
    """No device is touched: every answer here comes from the checks in front of the first launch (there is no GPU)."""
    import fosvos_hip
    L = fosvos_hip.lib()
    buf = ctypes.create_string_buffer(1 << 16)
    p = (ctypes.addressof(buf) + 255) // 256 * 256
    big = 1 << 40
    assert L.fosvos_distance_gate_workspace_bytes(1, 480, 854) == 16 + 2 * 480 * 854
    assert L.fosvos_adapt_labels_workspace_bytes(3, 480, 854) == 16 + 2 * 3 * 480 * 854 + 3 * 480 * 854
    for n, h, w in ((0, 4, 4), (65536, 4, 4), (1, 0, 4), (1, 4, 0), (1, 8193, 4), (1, 4, 8193)):
        assert L.fosvos_distance_gate_workspace_bytes(n, h, w) == 0 and L.fosvos_adapt_labels_workspace_bytes(n, h, w) == 0
        assert L.fosvos_distance_gate(p, n, h, w, 1, 0, p, p, big, 0, None) == E_SHAPE
        assert L.fosvos_adapt_labels(p, p, n, h, w, 1.0, 1, 0, p, p, p, p, big, 0, None) == E_SHAPE
    for d in (-1, 4096):
        assert L.fosvos_distance_gate(p, 1, 4, 4, d, 0, p, p, big, 0, None) == E_ARG
        assert L.fosvos_adapt_labels(p, p, 1, 4, 4, 1.0, d, 0, p, p, p, p, big, 0, None) == E_ARG
        assert L.fosvos_adapt_labels(p, p, 1, 4, 4, 1.0, 1, d, p, p, p, p, big, 0, None) == E_ARG
    assert L.fosvos_adapt_labels(p, p, 1, 4, 4, float("nan"), 1, 0, p, p, p, p, big, 0, None) == E_ARG
    assert L.fosvos_distance_gate(None, 1, 4, 4, 1, 0, p, p, big, 0, None) == E_ARG
    assert L.fosvos_distance_gate(p, 1, 4, 4, 1, 0, None, p, big, 0, None) == E_ARG
    assert L.fosvos_distance_gate(p, 1, 4, 4, 1, 0, p, None, big, 0, None) == E_ARG
    assert L.fosvos_distance_gate(p, 1, 4, 4, 1, 0, p, p + 8, big, 0, None) == E_ARG            # workspace off 16 bytes
    assert L.fosvos_distance_gate(p, 1, 4, 4, 1, 0, p, p, 16 + 2 * 16 - 1, 0, None) == E_WORKSPACE
    for k in range(6):
        args = [p, p, 1, 4, 4, 1.0, 1, 0, p, p, p, p, big, 0, None]
        args[(0, 1, 8, 9, 10, 11)[k]] = None
        assert L.fosvos_adapt_labels(*args) == E_ARG
    assert L.fosvos_adapt_labels(p, p, 1, 4, 4, 1.0, 1, 0, p, p, p, p, 16 + 32 + 16 - 1, 0, None) == E_WORKSPACE
    assert b"adapt_labels" in L.fosvos_last_error()
    # the void loss
    assert L.fosvos_cbce_workspace_bytes(480 * 854) == 3 * 1024 * 8              # unchanged
    assert L.fosvos_cbce_multi_workspace_bytes(480 * 854, 2, 5) == 10 * 3 * 1024 * 8
    assert L.fosvos_cbce_void_workspace_bytes(480 * 854, 2) == 2 * 4 * 1024 * 8
    need = L.fosvos_cbce_void_workspace_bytes(16, 1)
    ok = [p, p, p, 16, 1, 0, 1.0, p, p, p, big, 0, None]
    for k in (0, 1, 2, 7, 9):                                                    # logits, label, void, loss_out, workspace
        args = list(ok)
        args[k] = None
        assert L.fosvos_cbce_loss_frames_void(*args) == E_ARG, k
    for k, v in ((0, p + 4), (1, p + 8), (2, p + 2), (8, p + 4), (9, p + 4)):    # alignments
        args = list(ok)
        args[k] = v
        assert L.fosvos_cbce_loss_frames_void(*args) == E_ARG, k
    assert L.fosvos_cbce_loss_frames_void(p, p, p, 0, 1, 0, 1.0, p, p, p, big, 0, None) == E_SHAPE
    assert L.fosvos_cbce_loss_frames_void(p, p, p, 16, 0, 0, 1.0, p, p, p, big, 0, None) == E_SHAPE
    assert L.fosvos_cbce_loss_frames_void(p, p, p, 18, 2, 0, 1.0, p, p, p, big, 0, None) == E_SHAPE   # frames off 16 bytes
    assert L.fosvos_cbce_loss_frames_void(p, p, p, 16, 1, 0, 1.0, p, p, p, need - 1, 0, None) == E_WORKSPACE
    assert b"cbce_loss_frames_void" in L.fosvos_last_error()
