"""The CRF on the frame on a real MI355X: ``ops.crf_refine`` (csrc/crf.hip) against the numpy definition (util/mask_crf.py) bit
for bit - no tolerance anywhere -, the entry on islands, its argument faults, and ``test_fast(crf=)`` / ``test_objects(crf=)`` on
the real seeded OSVOS_VGG: files, score and the order of the calls.  tests/mask_crf_cases.py holds the shapes, the guides and
the definition's answers, each computed once."""
import contextlib
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import islands as I  # noqa: E402
import mask_crf_cases as C  # noqa: E402
import test_ensemble_cases as EC  # noqa: E402
import test_gpu_test_pass_calls as PC  # noqa: E402
from util import experiment_helper, mask_crf as M  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
NO_CPU = "tensor must live on the GPU (the HIP path has no CPU fallback)"


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)      # a copy: the shared references are read-only


# ------------------------------------------------------------------------------------------ the op against the definition
@pytest.mark.parametrize("guide", C.GUIDES)
@pytest.mark.parametrize("case", C.GPU_CASES, ids=C.IDS)
def test_op_is_the_definition(case, guide):
    from fosvos_hip import ops
    n, h, w, r = case
    missed = []
    for iterations in C.ITERATIONS:
        im, x, o, tab, want = C.reference(case, guide, iterations)
        assert np.array_equal(ops._crf_tables(o, torch.device(DEV)).cpu().numpy(), tab)     # the same table vector
        image_t, logits_t = dev(im), dev(x)
        got = ops.crf_refine(image_t, logits_t, o)
        assert tuple(got.shape) == (n, 1, h, w) and got.dtype == F32
        msg = C.same_bits(got.cpu().numpy(), want)
        if msg is not None:
            missed.append("%d iterations: %s" % (iterations, msg))
        assert np.array_equal(image_t.cpu().numpy(), im, equal_nan=True) and np.array_equal(logits_t.cpu().numpy(), x, equal_nan=True)
    assert not missed, (case, guide, missed)


def test_the_salt_case_reaches_the_empty_appearance_kernel():
    """What makes the 'salt' guide a case: on the host the branch ``Da == 0`` is taken at exactly the salt pixels."""
    n, h, w, r = C.GPU_CASES[3]
    im, x, o, tab, _ = C.reference(C.GPU_CASES[3], "salt", 1)
    _, da = M.messages(im[0], x[0, 0], o, tab)
    assert np.array_equal(da == 0.0, C.salt_frames(n, h, w)[0, :, :, 0] == 255) and (da == 0.0).sum() >= 6


def test_both_weights_zero_gives_the_clipped_logit():
    from fosvos_hip import ops
    case = C.GPU_CASES[4]
    im, x, o, _, want = C.reference(case, "random", 2, weights=(0.0, 0.0))
    got = ops.crf_refine(dev(im), dev(x), o).cpu().numpy()
    assert C.same_bits(got, want) is None, C.same_bits(got, want)
    xc = x.astype(np.float64)
    assert np.array_equal(got, np.where(np.isnan(xc), -6.0, np.clip(xc, -6.0, 6.0)).astype(np.float32))


def test_op_writes_into_the_callers_tensor_and_keeps_its_tables():
    from fosvos_hip import ops
    case = C.GPU_CASES[7]
    n, h, w, r = case
    im, x, o, _, want = C.reference(case, "random", 2)
    into = torch.full((n, 1, h, w), float("nan"), device=DEV)
    assert ops.crf_refine(dev(im), dev(x), o, out=into) is into
    assert C.same_bits(into.cpu().numpy(), want) is None
    assert ops._crf_tables(o, torch.device(DEV)) is ops._crf_tables(C.options(r, 2), torch.device(DEV))
    default = ops.crf_refine(dev(im), dev(x)).cpu().numpy()
    assert C.same_bits(default, M.refine_batch(im, x)) is None


# ------------------------------------------------------------------------------------------ islands
def test_the_entry_touches_nothing_outside_its_operands():
    """Three iterations - both maps of the workspace are written and read - with the workspace at exactly
    ``fosvos_crf_refine_workspace_bytes``."""
    import fosvos_hip
    from fosvos_hip import check, ops
    L = fosvos_hip.lib()
    case = (2, 19, 70, 3)
    n, h, w, r = case
    im, x, o, tab, want = C.reference(case, "nonfinite", 3)
    stream = torch.cuda.current_stream(0).cuda_stream
    need = int(L.fosvos_crf_refine_workspace_bytes(n, h, w))
    assert need == 2 * 8 * n * h * w
    operands = [I.inp("image", torch.from_numpy(im), is_map=False, offset=4), I.inp("logits", torch.from_numpy(x), is_map=False, offset=8),
                I.inp("tables", torch.from_numpy(tab), is_map=False, offset=8), I.out("out", (n, 1, h, w), F32, is_map=False, offset=12),
                I.workspace("workspace", need, offset=8)]

    def call(isl):
        check(L.fosvos_crf_refine(isl.ptr("image"), isl.ptr("logits"), isl.ptr("tables"), n, h, w, o.iterations, r,
                                  o.weight_appearance, o.weight_smooth, o.clip, ops._mean_bgr(), isl.ptr("out"), isl.ptr("workspace"),
                                  need, 0, stream), "crf_refine")

    I.run_case("crf_refine 2x19x70 r3, three iterations", operands, call, {"out": torch.from_numpy(want)}, device=DEV, seed=3).check()


# ------------------------------------------------------------------------------------------ argument faults
class LibRecorder:
    """``ops.lib()`` replaced: the launches (every entry that is no ``*_bytes`` query) are counted and forwarded."""

    def __init__(self, real):
        self.real, self.launches = real, []

    def __getattr__(self, name):
        fn = getattr(self.real, name)

        def call(*args):
            if not name.endswith("_bytes"):
                self.launches.append(name)
            return fn(*args)
        return call


@contextlib.contextmanager
def recording():
    import fosvos_hip
    from fosvos_hip import ops
    rec = LibRecorder(fosvos_hip.lib())
    saved = ops.lib
    ops.lib = lambda: rec
    try:
        yield rec
    finally:
        ops.lib = saved


def strided(t):
    return torch.stack([t, t], dim=-1)[..., 0]


def test_a_fault_raises_before_any_launch():
    from fosvos_hip import ops
    from fosvos_hip.options import CrfOptions
    n, h, w = 2, 12, 20
    image, logits = dev(C.image(n, h, w, "random")), dev(C.logits(n, h, w))
    new = lambda shape, dtype=F32: torch.empty(shape, dtype=dtype, device=DEV)  # noqa: E731
    both = torch.empty(n * 4 * h * w, device=DEV)
    cr = "crf_refine"
    rows = [
        ("image cpu", lambda: ops.crf_refine(image.cpu(), logits), RuntimeError, f"{cr} image: {NO_CPU}"),
        ("image dtype", lambda: ops.crf_refine(image.double(), logits), ValueError, f"{cr} image: expected torch.float32, got torch.float64"),
        ("image strided", lambda: ops.crf_refine(strided(image), logits), ValueError, f"{cr} image: tensor must be contiguous"),
        ("image shape", lambda: ops.crf_refine(image[:, :1].contiguous(), logits), ValueError,
         f"{cr}: image must be a non-empty [N,3,H,W], got {(n, 1, h, w)}"),
        ("image empty", lambda: ops.crf_refine(new((0, 3, h, w)), logits), ValueError,
         f"{cr}: image must be a non-empty [N,3,H,W], got {(0, 3, h, w)}"),
        ("image side", lambda: ops.crf_refine(new((1, 3, 1, 8193)), new((1, 1, 1, 8193))), ValueError,
         f"{cr}: maps may have sides of up to 8192, got {(1, 8193)}"),
        ("logits cpu", lambda: ops.crf_refine(image, logits.cpu()), RuntimeError, f"{cr} logits: {NO_CPU}"),
        ("logits dtype", lambda: ops.crf_refine(image, logits.double()), ValueError, f"{cr} logits: expected torch.float32, got torch.float64"),
        ("logits strided", lambda: ops.crf_refine(image, strided(logits)), ValueError, f"{cr} logits: tensor must be contiguous"),
        ("logits shape", lambda: ops.crf_refine(image, logits[:, 0].contiguous()), ValueError,
         f"{cr}: logits must be {(n, 1, h, w)}, got {(n, h, w)}"),
        ("logits size", lambda: ops.crf_refine(image, new((n, 1, h, w + 1))), ValueError,
         f"{cr}: logits must be {(n, 1, h, w)}, got {(n, 1, h, w + 1)}"),
        ("options", lambda: ops.crf_refine(image, logits, {"radius": 2}), ValueError,
         f"{cr}: options must be a fosvos_hip.options.CrfOptions or None, got {{'radius': 2}}"),
        ("radius", lambda: ops.crf_refine(image, logits, CrfOptions(radius=6)), ValueError,
         "CrfOptions: radius must be an integer in 1..5, got 6"),
        ("iterations", lambda: ops.crf_refine(image, logits, CrfOptions(iterations=11)), ValueError,
         "CrfOptions: iterations must be an integer in 1..10, got 11"),
        ("clip", lambda: ops.crf_refine(image, logits, CrfOptions(clip=0.0)), ValueError,
         "CrfOptions: clip must be a finite number in (0, 10000], got 0.0"),
        ("out shape", lambda: ops.crf_refine(image, logits, out=new((n, h, w))), ValueError, f"{cr}: out must be {(n, 1, h, w)}, got {(n, h, w)}"),
        ("out dtype", lambda: ops.crf_refine(image, logits, out=new((n, 1, h, w), F64)), ValueError,
         f"{cr} out: expected torch.float32, got torch.float64"),
        ("out cpu", lambda: ops.crf_refine(image, logits, out=torch.empty((n, 1, h, w))), RuntimeError, f"{cr} out: {NO_CPU}"),
        ("out is the logits", lambda: ops.crf_refine(image, logits, out=logits), ValueError,
         f"{cr}: out must not overlap the image or the logits"),
        ("out in the image", lambda: ops.crf_refine(both[:n * 3 * h * w].view(n, 3, h, w), logits,
                                                    out=both[n * 2 * h * w:n * 3 * h * w].view(n, 1, h, w)), ValueError,
         f"{cr}: out must not overlap the image or the logits"),
    ]
    missed = []
    for label, call, error, message in rows:
        with recording() as rec:
            try:
                call()
                got = "no exception"
            except Exception as e:  # noqa: BLE001  (the row names the one it expects)
                got = (type(e), str(e))
        if got != (error, message) or rec.launches:
            missed.append(f"{label}: expected {(error, message)}, got {got}, launches {rec.launches}")
    assert not missed, "\n".join(missed)
    with recording() as rec:
        ops.crf_refine(image, logits, CrfOptions(iterations=4))
        assert rec.launches == ["fosvos_crf_refine"]


def test_the_c_entry_refuses_its_faults_with_a_code_and_a_message():
    import fosvos_hip
    from fosvos_hip import ops
    L = fosvos_hip.lib()
    E_SHAPE, E_ARG = -1, -2
    n, h, w = 1, 4, 8
    image, logits, out = dev(C.image(n, h, w, "random")), dev(C.logits(n, h, w)), torch.empty((n, 1, h, w), device=DEV)
    tab = dev(M.tables())
    need = int(L.fosvos_crf_refine_workspace_bytes(n, h, w))
    ws = torch.empty(need + 8, dtype=torch.uint8, device=DEV)
    mean = ops._mean_bgr()

    def entry(image=image.data_ptr(), logits=logits.data_ptr(), tab=tab.data_ptr(), n=n, h=h, w=w, iterations=5, radius=5, wa=4.0,
              ws_=3.0, clip=6.0, mean=mean, out=out.data_ptr(), work=ws.data_ptr(), nbytes=need):
        return lambda: L.fosvos_crf_refine(image, logits, tab, n, h, w, iterations, radius, wa, ws_, clip, mean, out, work, nbytes, 0, None)

    null = "crf_refine: null pointer"
    cases = [
        (entry(image=None), E_ARG, null), (entry(logits=None), E_ARG, null), (entry(tab=None), E_ARG, null),
        (entry(mean=None), E_ARG, null), (entry(out=None), E_ARG, null), (entry(work=None), E_ARG, null),
        (entry(n=0), E_SHAPE, "crf_refine: N=0, maps of 4x8 (sides of 1..8192)"),
        (entry(h=8193), E_SHAPE, "crf_refine: N=1, maps of 8193x8 (sides of 1..8192)"),
        (entry(w=0), E_SHAPE, "crf_refine: N=1, maps of 4x0 (sides of 1..8192)"),
        (entry(iterations=0), E_ARG, "crf_refine: 0 iterations outside [1, 10]"),
        (entry(iterations=11), E_ARG, "crf_refine: 11 iterations outside [1, 10]"),
        (entry(radius=0), E_ARG, "crf_refine: radius 0 outside [1, 5]"),
        (entry(radius=6), E_ARG, "crf_refine: radius 6 outside [1, 5]"),
        (entry(wa=-1.0), E_ARG, "crf_refine: weights -1 and 3 outside [0, 100]"),
        (entry(ws_=float("nan")), E_ARG, "crf_refine: weights 4 and nan outside [0, 100]"),
        (entry(clip=0.0), E_ARG, "crf_refine: clip 0 outside (0, 1e4]"),
        (entry(clip=float("nan")), E_ARG, "crf_refine: clip nan outside (0, 1e4]"),
        (entry(out=out.data_ptr() + 2), E_ARG, "crf_refine: the image, the logits and out must be 4-byte aligned"),
        (entry(work=ws.data_ptr() + 4), E_ARG, "crf_refine: the tables and the workspace must be 8-byte aligned"),
        (entry(nbytes=need - 1), E_ARG, "crf_refine: workspace of %d bytes, need %d" % (need - 1, need)),
    ]
    assert L.fosvos_crf_refine_workspace_bytes(0, h, w) == 0 and L.fosvos_crf_refine_workspace_bytes(n, h, 8193) == 0
    torch.cuda.synchronize()
    with fosvos_hip.LaunchProfile(0) as prof:
        got = [(call(), L.fosvos_last_error().decode()) for call, _, _ in cases]
    assert got == [(code, message) for _, code, message in cases]
    assert prof.records == {}


# ------------------------------------------------------------------------------------------ the passes on the real net
SIZE = PC.SIZE


def crf_options():
    from fosvos_hip.options import CrfOptions
    return CrfOptions(iterations=3, radius=4)


class Recorder(PC.Recorder):
    """The recorder of tests/test_gpu_test_pass_calls.py with the CRF and the ensemble ops logged as well."""

    @contextlib.contextmanager
    def active(self, monkeypatch):
        from fosvos_hip import ops
        with super().active(monkeypatch):
            with monkeypatch.context() as m:
                for name in ("ensemble_views", "ensemble_merge", "crf_refine"):
                    m.setattr(ops, name, self._op(name, getattr(ops, name)))
                yield self


def by_definition(provider, crf, views=None):
    """The provider's net behind the numpy definition: what a pass with ``crf`` (behind an ensemble of ``views``) must equal."""
    net = provider.network if views is None else EC.EnsembleByDefinition(provider.network, views, device=DEV)
    return C.Provider(C.CrfByDefinition(net, crf, device=DEV))


@pytest.mark.parametrize("extra", ["alone", "clean", "ensemble"])
def test_fast_with_a_crf_writes_the_definitions_files(extra, tmp_path):
    """4 frames of 48x80 in groups of 3 and 1, two frames a forward call - which keeps each frame's arithmetic, so the
    comparison with the host pipeline of the same logits is byte for byte."""
    from fosvos_hip.options import CleanOptions, EnsembleOptions
    crf = crf_options()
    kw = {"clean": CleanOptions(largest=True)} if extra == "clean" else {}
    ens = EnsembleOptions(flip=True, scales=(0.75, 1.0)) if extra == "ensemble" else None
    prov = PC.Provider(PC.Recorder())
    loader = PC.blob_loader(4)
    score = experiment_helper.test_fast(prov, loader, tmp_path / "crf", loader.dataset.annotation, group=3, forward_batch=2,
                                        seq_name="blob", crf=crf, **kw, **({"ensemble": ens} if ens else {}))
    assert score["crf"] == crf.as_dict() == experiment_helper.last_fast["crf"]
    assert experiment_helper.last_fast["group_sizes"] == [3, 1]
    loader = PC.blob_loader(4)
    want = experiment_helper.test_fast(by_definition(prov, crf, None if ens is None else ens.views()), loader, tmp_path / "definition",
                                       loader.dataset.annotation, group=3, forward_batch=2, seq_name="blob", **kw)
    files = C.files_of(tmp_path / "crf")
    assert sorted(files) == ["blob/%05d.png" % k for k in range(4)]
    assert files == C.files_of(tmp_path / "definition")
    for key in ("counts", "J", "F", "J_stats", "F_stats", "J&F", "fnames", "scored"):
        assert score[key] == want[key], key
    assert "crf" not in want


def test_fast_without_a_crf_is_the_unchanged_call(tmp_path):
    prov = PC.Provider(PC.Recorder())
    crf = crf_options()
    runs = {}
    for name, kw in (("none", {"crf": None}), ("absent", {}), ("crf", {"crf": crf})):
        loader = PC.blob_loader(3)
        runs[name] = experiment_helper.test_fast(prov, loader, tmp_path / name, loader.dataset.annotation, group=2, seq_name="blob", **kw)
        if name != "crf":
            assert "crf" not in runs[name] and "crf" not in experiment_helper.last_fast
    assert C.files_of(tmp_path / "none") == C.files_of(tmp_path / "absent") != C.files_of(tmp_path / "crf")
    assert runs["none"]["counts"] == runs["absent"]["counts"]


def test_objects_with_a_crf_writes_the_definitions_files(tmp_path):
    from dataloaders.synthetic import SyntheticObjectsSequence
    from torch.utils.data import DataLoader
    crf = crf_options()
    rec = PC.Recorder()
    providers = [PC.Provider(rec, seed=2, name="forward net 1"), PC.Provider(rec, seed=3, name="forward net 2")]
    data = SyntheticObjectsSequence("blobs", SIZE[0], SIZE[1], n_frames=4, n_objects=2)

    def loader():
        return DataLoader(data, batch_size=1, shuffle=False, num_workers=0)

    score = experiment_helper.test_objects(providers, loader(), tmp_path / "crf", data.annotation, group=3, forward_batch=2,
                                           seq_name="blobs", crf=crf)
    want = experiment_helper.test_objects([by_definition(p, crf) for p in providers], loader(), tmp_path / "definition",
                                          data.annotation, group=3, forward_batch=2, seq_name="blobs")
    files = C.files_of(tmp_path / "crf")
    assert sorted(files) == ["blobs/%05d.png" % k for k in range(4)] and files == C.files_of(tmp_path / "definition")
    assert score["crf"] == crf.as_dict() and "crf" not in want
    assert [o["counts"] for o in score["objects"]] == [o["counts"] for o in want["objects"]]
    assert score["J&F"] == want["J&F"] and score["n_objects"] == 2


def test_fast_call_order(tmp_path, monkeypatch):
    """5 frames in groups of 3 and 2 with an ensemble and cleaning: per group the merge, ONE ``crf_refine``, the cleaning, then
    the sequence as without a CRF - and no host wait beyond that one's."""
    from fosvos_hip import ops
    from fosvos_hip.options import CleanOptions, EnsembleOptions
    crf = crf_options()
    ops._crf_tables(crf, torch.device(DEV))      # the one upload of these options' tables
    rec = Recorder()
    prov = PC.Provider(rec)
    loader = PC.blob_loader(5)
    with rec.active(monkeypatch):
        experiment_helper.test_fast(prov, loader, tmp_path / "a", loader.dataset.annotation, group=3, forward_batch=2, seq_name="blob",
                                    crf=crf, ensemble=EnsembleOptions(flip=True), clean=CleanOptions(largest=True))
    expected = []
    for g, n in enumerate([3, 2]):
        forwards = [("forward", min(2, n - k)) for _ in range(2) for k in range(0, n, 2)]
        expected += [("ensemble_views", ())] + forwards + [("ensemble_merge", ()), ("crf_refine", ()), ("clean_components", ("out",))]
        expected += [("jf_counts", ("out",)), ("prob_bytes", ()), ("png_encode", ("out", "lengths"))]
        expected += [PC.EVENT_WAIT] if g > 0 else []
    expected += [PC.EVENT_WAIT, PC.READ_BACK]
    assert rec.log == expected
    # without a CRF the op is not called: the sequence tests/test_gpu_test_pass_calls.py pins
    rec = Recorder()
    prov = PC.Provider(rec)
    loader = PC.blob_loader(5)
    with rec.active(monkeypatch):
        experiment_helper.test_fast(prov, loader, tmp_path / "b", loader.dataset.annotation, group=2, seq_name="blob")
    assert rec.log == PC.fast_expected([2, 2, 1], True)


def test_objects_call_order(tmp_path, monkeypatch):
    """2 nets, 3 frames in groups of 2 and 1: each net's logits are refined once a group, before the label merge."""
    from dataloaders.synthetic import SyntheticObjectsSequence
    from fosvos_hip import ops
    from torch.utils.data import DataLoader
    crf = crf_options()
    ops._crf_tables(crf, torch.device(DEV))
    data = SyntheticObjectsSequence("blobs", SIZE[0], SIZE[1], n_frames=3, n_objects=2)
    rec = Recorder()
    providers = [PC.Provider(rec, seed=2, name="forward net 1"), PC.Provider(rec, seed=3, name="forward net 2")]
    with rec.active(monkeypatch):
        experiment_helper.test_objects(providers, DataLoader(data, batch_size=1, shuffle=False, num_workers=0), tmp_path,
                                       data.annotation, group=2, seq_name="blobs", crf=crf)
    tail = [("merge_objects", ()), ("jf_counts_labels", ("out",)), ("png_encode_indexed", ("out", "lengths"))]
    expected = []
    for g, n in enumerate([2, 1]):
        expected += [("forward net 1", n), ("forward net 2", n), ("crf_refine", ()), ("crf_refine", ())]
        expected += tail + ([PC.EVENT_WAIT] if g > 0 else [])
    assert rec.log == expected + [PC.EVENT_WAIT, PC.READ_BACK]
