"""The joint CRF over the objects of a frame on a real MI355X: ``ops.crf_labels`` (csrc/crf.hip) against the numpy definition
(util/label_crf.py) - the labels equal, the scores bit for bit, no tolerance anywhere -, both weights 0 against
``ops.merge_objects``, the entry on islands, its argument faults, and ``test_objects(crf=, crf_joint=True)`` on the real seeded
OSVOS_VGG: files, counts, score and the order of the calls.  tests/label_crf_cases.py holds the shapes, the logit maps and the
definition's answers, each computed once."""
import contextlib
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import islands as I  # noqa: E402
import label_crf_cases as L  # noqa: E402
import mask_crf_cases as C  # noqa: E402
import test_gpu_mask_crf as GM  # noqa: E402
import test_gpu_test_pass_calls as PC  # noqa: E402
from util import experiment_helper, label_crf as LC  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64, U8 = torch.float32, torch.float64, torch.uint8
NO_CPU = GM.NO_CPU
dev = GM.dev


def devs(maps):
    return [dev(x) for x in maps]


# ------------------------------------------------------------------------------------------ the op against the definition
@pytest.mark.parametrize("guide", L.GUIDES)
@pytest.mark.parametrize("case", L.GPU_CASES, ids=L.IDS)
def test_op_is_the_definition(case, guide):
    from fosvos_hip import ops
    n, h, w, r, k = case
    missed = []
    for iterations in L.ITERATIONS:
        im, maps, o, tab, want_labels, want_scores = L.reference(case, guide, iterations)
        assert np.array_equal(ops._crf_tables(o, torch.device(DEV), labels=True).cpu().numpy(), tab)     # the same table vector
        image_t, maps_t = dev(im), devs(maps)
        scores = torch.full((n, k + 1, h, w), float("nan"), device=DEV)
        labels = ops.crf_labels(image_t, maps_t, o, scores=scores)
        assert tuple(labels.shape) == (n, h, w) and labels.dtype == U8
        if not np.array_equal(labels.cpu().numpy(), want_labels):
            bad = labels.cpu().numpy() != want_labels
            missed.append("%d iterations: %d of %d labels differ, first at %s" % (iterations, bad.sum(), bad.size, np.argwhere(bad)[0]))
        msg = C.same_bits(scores.cpu().numpy(), want_scores)
        if msg is not None:
            missed.append("%d iterations: scores: %s" % (iterations, msg))
        # without the scores the labels are the same, and no input was written
        assert torch.equal(ops.crf_labels(image_t, maps_t, o), labels)
        assert np.array_equal(image_t.cpu().numpy(), im, equal_nan=True)
        assert all(np.array_equal(t.cpu().numpy(), x, equal_nan=True) for t, x in zip(maps_t, maps))
    assert not missed, (case, guide, missed)


def test_the_cases_plant_ties_across_the_nets():
    """What makes ``logit_maps`` a case: pixels where all nets hold one value, and pixels where the last two lead with one."""
    maps = np.stack(L.logit_maps(2, 19, 70, 3))
    assert ((maps == maps[:1]).all(axis=0) & (maps[0] > 0)).sum() >= 4 and np.isnan(maps).all(axis=0).sum() >= 2
    assert ((maps[1] == maps[2]) & (maps[1] > maps[0]) & (maps[1] == 5.5)).sum() >= 2
    _, _, _, _, labels, scores = L.reference((2, 19, 70, 3, 3), "constant", 1, weights=(0.0, 0.0))
    lead = (maps[1] == 5.5) & (maps[2] == 5.5) & (maps[0] < 5.5)
    assert (labels[lead[:, 0]] == 2).all()


@pytest.mark.parametrize("k", [1, 3, 16])
def test_both_weights_zero_is_merge_objects(k):
    """The same tensors through both ops.  With the widest clip every finite logit of the case is inside it; +-inf are the clip
    itself and a NaN is never an object, in both."""
    from fosvos_hip import ops
    from fosvos_hip.options import CrfOptions
    n, h, w = 2, 19, 70
    o = CrfOptions(iterations=2, radius=3, weight_appearance=0.0, weight_smooth=0.0, clip=1e4)
    maps = [np.where(x > 1e4, np.float32(np.inf), np.where(x < -1e4, np.float32(-np.inf), x)) for x in L.logit_maps(n, h, w, k)]
    assert any(np.isinf(x).any() for x in maps) and any(np.isnan(x).any() for x in maps)
    maps_t = devs(maps)
    got = ops.crf_labels(dev(C.image(n, h, w, "random")), maps_t, o)
    assert torch.equal(got, ops.merge_objects(maps_t))
    assert len(np.unique(got.cpu().numpy())) == k + 1


def test_op_writes_into_the_callers_views_and_keeps_its_tables():
    from fosvos_hip import ops
    case = L.GPU_CASES[7]
    n, h, w, r, k = case
    im, maps, o, _, want_labels, want_scores = L.reference(case, "random", 2)
    holder = torch.full((n + 2, h, w), 0xEE, dtype=U8, device=DEV)
    score_holder = torch.full((2, n, k + 1, h, w), float("nan"), device=DEV)
    into, scores = holder[1:1 + n], score_holder[1]
    assert ops.crf_labels(dev(im), devs(maps), o, out=into, scores=scores) is into
    assert np.array_equal(into.cpu().numpy(), want_labels) and C.same_bits(scores.cpu().numpy(), want_scores) is None
    assert (holder[0] == 0xEE).all() and (holder[-1] == 0xEE).all() and torch.isnan(score_holder[0]).all()
    device = torch.device(DEV)
    assert ops._crf_tables(o, device, labels=True) is ops._crf_tables(C.options(r, 2), device, labels=True)
    assert ops._crf_tables(o, device, labels=True) is not ops._crf_tables(o, device)         # a key of its own
    default = ops.crf_labels(dev(im), devs(maps)).cpu().numpy()
    assert np.array_equal(default, LC.refine_labels_batch(im, maps)[0])


# ------------------------------------------------------------------------------------------ islands
def test_the_entry_touches_nothing_outside_its_operands():
    """Three iterations - both sets of the workspace are written and read - with the workspace at exactly
    ``fosvos_crf_labels_workspace_bytes``."""
    import fosvos_hip
    from fosvos_hip import check, ops
    lib = fosvos_hip.lib()
    case = (2, 19, 70, 3, 3)
    n, h, w, r, k = case
    im, maps, o, tab, want_labels, want_scores = L.reference(case, "nonfinite", 3)
    stream = torch.cuda.current_stream(0).cuda_stream
    need = int(lib.fosvos_crf_labels_workspace_bytes(n, k, h, w))
    assert need == 16 * (k + 1) * n * h * w
    operands = [I.inp("image", torch.from_numpy(im), is_map=False, offset=4), I.inp("tables", torch.from_numpy(tab), is_map=False, offset=8)]
    operands += [I.inp("logits%d" % j, torch.from_numpy(x), is_map=False, offset=4 * (j + 1)) for j, x in enumerate(maps)]
    operands += [I.out("labels", (n, h, w), U8, is_map=False, offset=1), I.out("scores", (n, k + 1, h, w), F32, is_map=False, offset=12),
                 I.workspace("workspace", need, offset=8)]

    def call(isl):
        table = (ctypes.c_void_p * k)(*[isl.ptr("logits%d" % j) for j in range(k)])
        check(lib.fosvos_crf_labels(isl.ptr("image"), table, k, isl.ptr("tables"), n, h, w, o.iterations, r, o.weight_appearance,
                                    o.weight_smooth, o.clip, ops._mean_bgr(), isl.ptr("labels"), isl.ptr("scores"),
                                    isl.ptr("workspace"), need, 0, stream), "crf_labels")

    I.run_case("crf_labels 2x19x70 r3 K3, three iterations", operands, call,
               {"labels": torch.from_numpy(want_labels), "scores": torch.from_numpy(want_scores)}, device=DEV, seed=3).check()


# ------------------------------------------------------------------------------------------ argument faults
def test_a_fault_raises_before_any_launch():
    from fosvos_hip import ops
    from fosvos_hip.options import CrfOptions
    n, h, w, k = 2, 12, 20, 2
    image, logits = dev(C.image(n, h, w, "random")), devs(L.logit_maps(n, h, w, k))
    new = lambda shape, dtype=F32: torch.empty(shape, dtype=dtype, device=DEV)  # noqa: E731
    cl = "crf_labels"
    one = logits[0]
    shared = torch.empty(n * h * w * 2, device=DEV)
    rows = [
        ("image cpu", lambda: ops.crf_labels(image.cpu(), logits), RuntimeError, f"{cl} image: {NO_CPU}"),
        ("image dtype", lambda: ops.crf_labels(image.double(), logits), ValueError, f"{cl} image: expected torch.float32, got torch.float64"),
        ("image strided", lambda: ops.crf_labels(GM.strided(image), logits), ValueError, f"{cl} image: tensor must be contiguous"),
        ("image shape", lambda: ops.crf_labels(image[:, :1].contiguous(), logits), ValueError,
         f"{cl}: image must be a non-empty [N,3,H,W], got {(n, 1, h, w)}"),
        ("image side", lambda: ops.crf_labels(new((1, 3, 1, 8193)), [new((1, 1, 1, 8193))]), ValueError,
         f"{cl}: maps may have sides of up to 8192, got {(1, 8193)}"),
        ("no logits", lambda: ops.crf_labels(image, []), ValueError, f"{cl}: 0 logit maps, outside [1, 16]"),
        ("17 logits", lambda: ops.crf_labels(image, [one] * 17), ValueError, f"{cl}: 17 logit maps, outside [1, 16]"),
        ("logits cpu", lambda: ops.crf_labels(image, [one, one.cpu()]), RuntimeError, f"{cl} logits: {NO_CPU}"),
        ("logits dtype", lambda: ops.crf_labels(image, [one.double()]), ValueError, f"{cl} logits: expected torch.float32, got torch.float64"),
        ("logits strided", lambda: ops.crf_labels(image, [GM.strided(one)]), ValueError, f"{cl} logits: tensor must be contiguous"),
        ("logits shape", lambda: ops.crf_labels(image, [one, one[:, 0].contiguous()]), ValueError,
         f"{cl}: every logit map must be {(n, 1, h, w)}, got {(n, h, w)}"),
        ("logits size", lambda: ops.crf_labels(image, [new((n, 1, h, w + 1))]), ValueError,
         f"{cl}: every logit map must be {(n, 1, h, w)}, got {(n, 1, h, w + 1)}"),
        ("options", lambda: ops.crf_labels(image, logits, {"radius": 2}), ValueError,
         f"{cl}: options must be a fosvos_hip.options.CrfOptions or None, got {{'radius': 2}}"),
        ("radius", lambda: ops.crf_labels(image, logits, CrfOptions(radius=6)), ValueError,
         "CrfOptions: radius must be an integer in 1..5, got 6"),
        ("out shape", lambda: ops.crf_labels(image, logits, out=new((n, 1, h, w), U8)), ValueError,
         f"{cl}: out must be {(n, h, w)}, got {(n, 1, h, w)}"),
        ("out dtype", lambda: ops.crf_labels(image, logits, out=new((n, h, w))), ValueError, f"{cl} out: expected torch.uint8, got torch.float32"),
        ("out cpu", lambda: ops.crf_labels(image, logits, out=torch.empty((n, h, w), dtype=U8)), RuntimeError, f"{cl} out: {NO_CPU}"),
        ("scores shape", lambda: ops.crf_labels(image, logits, scores=new((n, k, h, w))), ValueError,
         f"{cl}: scores must be {(n, k + 1, h, w)}, got {(n, k, h, w)}"),
        ("scores dtype", lambda: ops.crf_labels(image, logits, scores=new((n, k + 1, h, w), F64)), ValueError,
         f"{cl} scores: expected torch.float32, got torch.float64"),
        ("scores in a logit map", lambda: ops.crf_labels(image, [shared[:n * h * w].view(n, 1, h, w)],
                                                         scores=shared.view(n, 2, h, w)), ValueError,
         f"{cl}: out and scores must not overlap the image, the logits or each other"),
    ]
    missed = []
    for label, call, error, message in rows:
        with GM.recording() as rec:
            try:
                call()
                got = "no exception"
            except Exception as e:  # noqa: BLE001  (the row names the one it expects)
                got = (type(e), str(e))
        if got != (error, message) or rec.launches:
            missed.append(f"{label}: expected {(error, message)}, got {got}, launches {rec.launches}")
    assert not missed, "\n".join(missed)
    with GM.recording() as rec:
        ops.crf_labels(image, logits, CrfOptions(iterations=4))
        assert rec.launches == ["fosvos_crf_labels"]


def test_the_c_entry_refuses_its_faults_with_a_code_and_a_message():
    import fosvos_hip
    from fosvos_hip import ops
    lib = fosvos_hip.lib()
    E_SHAPE, E_ARG = -1, -2
    n, h, w, k = 1, 4, 8, 2
    image, maps = dev(C.image(n, h, w, "random")), devs(L.logit_maps(n, h, w, k))
    labels, scores = torch.empty((n, h, w), dtype=U8, device=DEV), torch.empty((n, k + 1, h, w), device=DEV)
    tab = dev(LC.tables())
    need = int(lib.fosvos_crf_labels_workspace_bytes(n, k, h, w))
    ws = torch.empty(need + 8, dtype=U8, device=DEV)
    mean = ops._mean_bgr()
    good = (ctypes.c_void_p * k)(*[t.data_ptr() for t in maps])
    holed = (ctypes.c_void_p * k)(maps[0].data_ptr(), None)
    odd = (ctypes.c_void_p * k)(maps[0].data_ptr(), maps[1].data_ptr() + 2)

    def entry(image=image.data_ptr(), table=good, k=k, tab=tab.data_ptr(), n=n, h=h, w=w, iterations=5, radius=5, wa=4.0, ws_=3.0,
              clip=6.0, mean=mean, labels=labels.data_ptr(), scores=scores.data_ptr(), work=ws.data_ptr(), nbytes=need):
        return lambda: lib.fosvos_crf_labels(image, table, k, tab, n, h, w, iterations, radius, wa, ws_, clip, mean, labels, scores,
                                             work, nbytes, 0, None)

    null = "crf_labels: null pointer"
    aligned = "crf_labels: the image, the logits and the scores must be 4-byte aligned"
    cases = [
        (entry(k=0), E_ARG, "crf_labels: K=0 outside [1, 16]"), (entry(k=17), E_ARG, "crf_labels: K=17 outside [1, 16]"),
        (entry(image=None), E_ARG, null), (entry(table=None), E_ARG, null), (entry(tab=None), E_ARG, null),
        (entry(mean=None), E_ARG, null), (entry(labels=None), E_ARG, null), (entry(work=None), E_ARG, null),
        (entry(n=0), E_SHAPE, "crf_labels: N=0, maps of 4x8 (sides of 1..8192)"),
        (entry(h=8193), E_SHAPE, "crf_labels: N=1, maps of 8193x8 (sides of 1..8192)"),
        (entry(iterations=0), E_ARG, "crf_labels: 0 iterations outside [1, 10]"),
        (entry(iterations=11), E_ARG, "crf_labels: 11 iterations outside [1, 10]"),
        (entry(radius=0), E_ARG, "crf_labels: radius 0 outside [1, 5]"),
        (entry(radius=6), E_ARG, "crf_labels: radius 6 outside [1, 5]"),
        (entry(wa=-1.0), E_ARG, "crf_labels: weights -1 and 3 outside [0, 100]"),
        (entry(ws_=float("nan")), E_ARG, "crf_labels: weights 4 and nan outside [0, 100]"),
        (entry(clip=0.0), E_ARG, "crf_labels: clip 0 outside (0, 1e4]"),
        (entry(table=holed), E_ARG, "crf_labels: null logit map 1"),
        (entry(table=odd), E_ARG, aligned), (entry(scores=scores.data_ptr() + 2), E_ARG, aligned),
        (entry(work=ws.data_ptr() + 4), E_ARG, "crf_labels: the tables and the workspace must be 8-byte aligned"),
        (entry(nbytes=need - 1), E_ARG, "crf_labels: workspace of %d bytes, need %d" % (need - 1, need)),
    ]
    query = lib.fosvos_crf_labels_workspace_bytes
    assert query(0, k, h, w) == 0 and query(n, 0, h, w) == 0 and query(n, 17, h, w) == 0 and query(n, k, h, 8193) == 0
    assert query(5, 16, 480, 854) == 16 * 17 * 5 * 480 * 854
    torch.cuda.synchronize()
    with fosvos_hip.LaunchProfile(0) as prof:
        got = [(call(), lib.fosvos_last_error().decode()) for call, _, _ in cases]
    assert got == [(code, message) for _, code, message in cases]
    assert prof.records == {}
    # a NULL for the scores is no fault: the labels alone
    assert entry(scores=None, iterations=2)() == 0
    torch.cuda.synchronize()
    want = LC.refine_labels_batch(image.cpu().numpy(), [t.cpu().numpy() for t in maps], C.options(5, 2))[0]
    assert np.array_equal(labels.cpu().numpy(), want)


# ------------------------------------------------------------------------------------------ the pass on the real net
SIZE = PC.SIZE


class Recorder(GM.Recorder):
    """The recorder of tests/test_gpu_mask_crf.py with the joint op logged as well."""

    @contextlib.contextmanager
    def active(self, monkeypatch):
        from fosvos_hip import ops
        with super().active(monkeypatch):
            with monkeypatch.context() as m:
                m.setattr(ops, "crf_labels", self._op("crf_labels", ops.crf_labels))
                yield self


def object_run(tmp_path, name, providers, n_frames=4, **kw):
    from dataloaders.synthetic import SyntheticObjectsSequence
    from torch.utils.data import DataLoader
    data = SyntheticObjectsSequence("blobs", SIZE[0], SIZE[1], n_frames=n_frames, n_objects=len(providers))
    return experiment_helper.test_objects(providers, DataLoader(data, batch_size=1, shuffle=False, num_workers=0), tmp_path / name,
                                          data.annotation, group=3, forward_batch=2, seq_name="blobs", **kw)


def test_objects_with_a_joint_crf_writes_the_definitions_files(tmp_path):
    """4 frames of 48x80 in groups of 3 and 1, two frames a forward call, two nets: the pass against the pass without a CRF
    over nets that answer with the definition's label maps (computed on the host from the same nets' logits)."""
    crf = GM.crf_options()
    rec = PC.Recorder()
    providers = [PC.Provider(rec, seed=2, name="forward net 1"), PC.Provider(rec, seed=3, name="forward net 2")]
    score = object_run(tmp_path, "joint", providers, crf=crf, crf_joint=True)
    inner = [p.network for p in providers]
    want = object_run(tmp_path, "definition", [C.Provider(L.JointByDefinition(inner, j, crf, device=DEV)) for j in range(2)])
    files = C.files_of(tmp_path / "joint")
    assert sorted(files) == ["blobs/%05d.png" % k for k in range(4)] and files == C.files_of(tmp_path / "definition")
    assert score["crf"] == crf.as_dict() and score["crf_joint"] is True and "crf" not in want and "crf_joint" not in want
    assert [o["counts"] for o in score["objects"]] == [o["counts"] for o in want["objects"]]
    assert score["J&F"] == want["J&F"] and score["n_objects"] == 2


def test_objects_without_the_argument_is_the_unchanged_call(tmp_path):
    crf = GM.crf_options()
    rec = PC.Recorder()
    providers = [PC.Provider(rec, seed=2, name="forward net 1"), PC.Provider(rec, seed=3, name="forward net 2")]
    runs = {name: object_run(tmp_path, name, providers, n_frames=3, **kw)
            for name, kw in (("false", {"crf": crf, "crf_joint": False}), ("absent", {"crf": crf}), ("joint", {"crf": crf, "crf_joint": True}))}
    assert "crf_joint" not in runs["false"] and "crf_joint" not in runs["absent"] and runs["joint"]["crf_joint"] is True
    assert C.files_of(tmp_path / "false") == C.files_of(tmp_path / "absent")
    assert [o["counts"] for o in runs["false"]["objects"]] == [o["counts"] for o in runs["absent"]["objects"]]


def test_objects_call_order(tmp_path, monkeypatch):
    """2 nets, 3 frames in groups of 2 and 1: with ``crf_joint`` ONE ``crf_labels`` a group in the place of the two
    ``crf_refine`` and of ``merge_objects``, and no host wait beyond the pass's own; without it the sequence
    tests/test_gpu_mask_crf.py pins."""
    from dataloaders.synthetic import SyntheticObjectsSequence
    from fosvos_hip import ops
    from torch.utils.data import DataLoader
    crf = GM.crf_options()
    ops._crf_tables(crf, torch.device(DEV), labels=True)      # the one upload of these options' tables
    ops._crf_tables(crf, torch.device(DEV))
    data = SyntheticObjectsSequence("blobs", SIZE[0], SIZE[1], n_frames=3, n_objects=2)
    logs = {}
    for name, kw in (("joint", {"crf_joint": True}), ("per net", {})):
        rec = Recorder()
        providers = [PC.Provider(rec, seed=2, name="forward net 1"), PC.Provider(rec, seed=3, name="forward net 2")]
        with rec.active(monkeypatch):
            experiment_helper.test_objects(providers, DataLoader(data, batch_size=1, shuffle=False, num_workers=0), tmp_path / name,
                                           data.annotation, group=2, seq_name="blobs", crf=crf, **kw)
        logs[name] = rec.log
    tail = [("jf_counts_labels", ("out",)), ("png_encode_indexed", ("out", "lengths"))]
    expected = {"joint": [], "per net": []}
    for g, n in enumerate([2, 1]):
        forwards = [("forward net 1", n), ("forward net 2", n)]
        wait = [PC.EVENT_WAIT] if g > 0 else []
        expected["joint"] += forwards + [("crf_labels", ())] + tail + wait
        expected["per net"] += forwards + [("crf_refine", ()), ("crf_refine", ()), ("merge_objects", ())] + tail + wait
    for name in logs:
        assert logs[name] == expected[name] + [PC.EVENT_WAIT, PC.READ_BACK], name
