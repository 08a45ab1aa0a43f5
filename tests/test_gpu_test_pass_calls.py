"""What the four sequence-level test passes of util/experiment_helper.py ask of the device, in order: the ``fosvos_hip.ops``
calls with the buffers they were handed, the nets' forward calls and the host waits.  The expected sequences are written out
below from each case's parameters; nothing here looks at a kernel, only at Python-level calls."""
import contextlib
import inspect
import os
import sys

import pytest
import torch

from oracle import osvos_ref as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))

from util import experiment_helper, io_helper  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZE = (48, 80)

OPS = ("prob_bytes", "png_encode", "png_encode_indexed", "jf_counts", "jf_counts_labels", "merge_objects", "clean_components",
       "adapt_labels")
BUFFERS = ("out", "lengths", "kept", "label", "void", "counts")
EVENT_WAIT = ("wait", "Event.synchronize")
READ_BACK = ("wait", "Tensor.cpu")


class Recorder:
    """The log of one call of a pass: ('forward', batch size), (op name, the buffer arguments that were passed) and
    ('wait', what waited).  Nothing is logged while a forward runs."""

    def __init__(self):
        self.log, self.quiet = [], 0

    def add(self, *entry):
        if not self.quiet:
            self.log.append(entry)

    @contextlib.contextmanager
    def active(self, monkeypatch):
        from fosvos_hip import ops
        with monkeypatch.context() as m:
            for name in OPS:
                m.setattr(ops, name, self._op(name, getattr(ops, name)))
            m.setattr(torch.cuda.Event, "synchronize", self._wait("Event.synchronize", torch.cuda.Event.synchronize))
            m.setattr(torch.cuda.Stream, "synchronize", self._wait("Stream.synchronize", torch.cuda.Stream.synchronize))
            m.setattr(torch.cuda, "synchronize", self._wait("cuda.synchronize", torch.cuda.synchronize))
            for name in ("cpu", "item", "tolist", "numpy"):
                m.setattr(torch.Tensor, name, self._read("Tensor." + name, getattr(torch.Tensor, name)))
            yield self

    def _op(self, name, original):
        signature = inspect.signature(original)

        def op(*args, **kwargs):
            given = signature.bind(*args, **kwargs).arguments
            self.add(name, tuple(b for b in BUFFERS if given.get(b) is not None))
            return original(*args, **kwargs)
        return op

    def _wait(self, what, original):
        def wait(*args, **kwargs):
            self.add("wait", what)
            return original(*args, **kwargs)
        return wait

    def _read(self, what, original):
        def read(tensor, *args, **kwargs):
            if tensor.is_cuda:  # (a read of pinned host memory waits for nothing)
                self.add("wait", what)
            return original(tensor, *args, **kwargs)
        return read


class Net(torch.nn.Module):
    """The real OSVOS_VGG forward with each frame's median taken off the fused logits (about half of the pixels are object),
    logged as one atom."""

    def __init__(self, net, recorder, name="forward"):
        super().__init__()
        self.net, self.recorder, self.name = net, recorder, name

    def forward(self, x):
        self.recorder.add(self.name, int(x.shape[0]))
        self.recorder.quiet += 1
        try:
            outs = list(self.net.forward(x))
            fused = outs[-1]
            outs[-1] = fused - fused.flatten(1).median(dim=1).values.view(-1, 1, 1, 1)
            return outs
        finally:
            self.recorder.quiet -= 1


class Provider:
    def __init__(self, recorder, seed=2, name="forward"):
        from networks.osvos_vgg import OSVOS_VGG
        from util.network_provider import VGGOnlineProvider
        net = OSVOS_VGG(pretrained=0)
        net.load_state_dict(O.make_state_dict(seed))
        self.inner = VGGOnlineProvider.__new__(VGGOnlineProvider)
        self.inner.network = net.to(DEV)
        self.network = Net(self.inner.network, recorder, name)
        self.optimizers = 0

    def get_optimizer(self, learning_rate=1e-8):
        self.optimizers += 1
        return self.inner.get_optimizer(learning_rate=learning_rate)


def blob_loader(n_frames):
    return io_helper.get_data_loader_test(None, 1, "blob", synthetic=SIZE, n_frames=n_frames)


def check_files_follow_one_group_behind(log, encode):
    """The wait for group g's files comes after group g + 1's encode call and before group g + 2's; after the last encode
    call one wait is left, the last group's; and from the first group's first call to that last wait the host waits for
    nothing else."""
    encodes = [k for k, entry in enumerate(log) if entry[0] == encode]
    waits = [k for k, entry in enumerate(log) if entry == EVENT_WAIT]
    assert len(encodes) >= 3 and len(waits) == len(encodes)
    for g, at in enumerate(waits[:-1]):
        assert encodes[g + 1] < at and (g + 2 >= len(encodes) or at < encodes[g + 2]), (g, at, encodes)
    assert waits[-1] > encodes[-1]
    assert [entry for entry in log[:waits[-1] + 1] if entry[0] == "wait"] == [EVENT_WAIT] * len(encodes)


def check_files_exist(save_dir, seq, fnames):
    assert len(fnames) and all((save_dir / seq / (name + ".png")).is_file() for name in fnames)


# ------------------------------------------------------------------------------------------ test_fast
def fast_expected(group_sizes, annotations, clean=()):
    log = []
    for g, n in enumerate(group_sizes):
        log.append(("forward", n))
        log += [("clean_components", clean)] if clean else []
        log += [("jf_counts", ("out",))] if annotations else []
        log += [("prob_bytes", ()), ("png_encode", ("out", "lengths"))]
        log += [EVENT_WAIT] if g > 0 else []       # the files of the group before
    log.append(EVENT_WAIT)                         # the last group's files
    log += [READ_BACK] if annotations else []      # the [n_frames,6] counters, once
    return log


@pytest.mark.parametrize("case", ["annotations", "no_annotations", "clean"])
def test_fast_calls(case, tmp_path, monkeypatch):
    """5 frames in groups of 2, 2 and 1, each forwarded in one call of its size."""
    rec = Recorder()
    prov = Provider(rec)
    loader = blob_loader(5)
    kw = {}
    if case == "clean":
        from fosvos_hip.options import CleanOptions
        kw = {"clean": CleanOptions(temporal_radius=1), "clean_seed": loader.dataset.annotation("blob", "00000")}
    annotations = None if case == "no_annotations" else loader.dataset.annotation
    with rec.active(monkeypatch):
        score = experiment_helper.test_fast(prov, loader, tmp_path, annotations, group=2, seq_name="blob", **kw)
    assert rec.log == fast_expected([2, 2, 1], annotations is not None, ("out", "kept") if case == "clean" else ())
    check_files_follow_one_group_behind(rec.log, "png_encode")
    assert experiment_helper.last_fast["group_sizes"] == [2, 2, 1]
    if annotations is None:
        assert score is None
        check_files_exist(tmp_path, "blob", ["%05d" % k for k in range(5)])
    else:
        assert score["fnames"] == ["%05d" % k for k in range(5)] and all(score["scored"])
        check_files_exist(tmp_path, "blob", score["fnames"])


# ------------------------------------------------------------------------------------------ test_objects
def test_objects_calls(tmp_path, monkeypatch):
    """2 nets, 5 frames in groups of 2, 2 and 1: both nets forward a group before anything else is asked for it."""
    from dataloaders.synthetic import SyntheticObjectsSequence
    from torch.utils.data import DataLoader
    rec = Recorder()
    providers = [Provider(rec, seed=2, name="forward net 1"), Provider(rec, seed=3, name="forward net 2")]
    data = SyntheticObjectsSequence("blobs", SIZE[0], SIZE[1], n_frames=5, n_objects=2)
    loader = DataLoader(data, batch_size=1, shuffle=False, num_workers=0)
    with rec.active(monkeypatch):
        score = experiment_helper.test_objects(providers, loader, tmp_path, data.annotation, group=2, seq_name="blobs")
    expected = []
    for g, n in enumerate([2, 2, 1]):
        expected += [("forward net 1", n), ("forward net 2", n), ("merge_objects", ()), ("jf_counts_labels", ("out",)),
                     ("png_encode_indexed", ("out", "lengths"))]
        expected += [EVENT_WAIT] if g > 0 else []
    expected += [EVENT_WAIT, READ_BACK]            # the last group's files; the [n_frames,2,6] counters, once
    assert rec.log == expected
    check_files_follow_one_group_behind(rec.log, "png_encode_indexed")
    assert score["n_objects"] == 2 and score["fnames"] == ["%05d" % k for k in range(5)]
    check_files_exist(tmp_path, "blobs", score["fnames"])


# ------------------------------------------------------------------------------------------ test_adaptive
@pytest.mark.parametrize("steps", [1, 0])
def test_adaptive_calls(steps, tmp_path, monkeypatch):
    """3 frames, one a group.  With a step a frame is forwarded twice outside the training step - which is one forward of
    the first frame and this one together, 48 x 80 being a multiple of 4 - and once without."""
    from fosvos_hip.options import AdaptOptions
    rec = Recorder()
    prov = Provider(rec)
    loader = blob_loader(3)
    train = io_helper.get_data_loader_train(None, 1, "blob", synthetic=SIZE)
    first = {"image": train.dataset[0]["image"], "gt": train.dataset[0]["gt"]}
    adapt = AdaptOptions(steps=steps, neg_distance=12, erode=2)
    with rec.active(monkeypatch):
        score = experiment_helper.test_adaptive(prov, loader, tmp_path, first, adapt, loader.dataset.annotation, seq_name="blob")
    expected = []
    for t in range(3):
        expected += [("forward", 1), ("adapt_labels", ("label", "void", "counts"))]
        expected += [("forward", 2), ("forward", 1)] * steps
        expected += [("jf_counts", ("out",)), ("prob_bytes", ()), ("png_encode", ("out", "lengths"))]
        expected += [EVENT_WAIT] if t > 0 else []
    expected += [EVENT_WAIT, READ_BACK, READ_BACK]  # the last file; the [n_frames,6] and the [n_frames,3] counters, once each
    assert rec.log == expected
    check_files_follow_one_group_behind(rec.log, "png_encode")
    assert prov.optimizers == steps
    assert score["fnames"] == ["%05d" % k for k in range(3)] and len(score["adapt"]["counts"]) == 3
    assert experiment_helper.last_fast["group_sizes"] == [1, 1, 1]
    check_files_exist(tmp_path, "blob", score["fnames"])


# ------------------------------------------------------------------------------------------ test_scored
def test_scored_calls(tmp_path, monkeypatch):
    """3 frames: the bytes of every minibatch are read back as they come, the counters once at the end."""
    rec = Recorder()
    prov = Provider(rec)
    loader = blob_loader(3)
    with rec.active(monkeypatch):
        score = experiment_helper.test_scored(prov, loader, tmp_path, loader.dataset.annotation, seq_name="blob")
    assert rec.log == [("forward", 1), ("jf_counts", ("out",)), ("prob_bytes", ()), READ_BACK] * 3 + [READ_BACK]
    assert score["fnames"] == ["%05d" % k for k in range(3)]
    check_files_exist(tmp_path, "blob", score["fnames"])
