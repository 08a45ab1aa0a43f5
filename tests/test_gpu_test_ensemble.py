"""The test-time ensemble on a real MI355X: ``ops.ensemble_views`` and ``ops.ensemble_merge`` (csrc/ensemble.hip) against the
numpy definition (util/test_ensemble.py) bit for bit, both entries on islands, their argument faults, and
``test_fast(ensemble=)`` / ``test_objects(ensemble=)`` on the real seeded OSVOS_VGG: files, score and the order of the calls.
tests/test_ensemble_cases.py holds the shapes, the view sets and the rule by which bits are compared."""
import contextlib
import ctypes
import os
import sys
import zlib

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import islands as I  # noqa: E402
import test_ensemble_cases as C  # noqa: E402
import test_gpu_test_pass_calls as PC  # noqa: E402
from util import experiment_helper, test_ensemble as TE  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
F, T = False, True
NO_CPU = "tensor must live on the GPU (the HIP path has no CPU fallback)"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def carved(shape, data=None):
    """A float32 tensor of ``shape`` on the device that starts one float past a 16-byte boundary."""
    numel = int(np.prod(shape))
    buf = torch.empty(numel + 8, dtype=F32, device=DEV)
    off = ((4 - buf.data_ptr() % 16) % 16) // 4
    t = buf[off:off + numel].view(*shape)
    assert t.data_ptr() % 16 == 4
    if data is not None:
        t.copy_(torch.from_numpy(np.ascontiguousarray(data)))
    return t


def check_views(got, image_t, x, views, tag):
    want = TE.make_views(x, views)
    h, w = x.shape[2:]
    assert len(got) == len(views)
    for k, ((scale, flip), g, v) in enumerate(zip(views, got, want)):
        if TE.view_sizes(h, w, scale) == (h, w) and not flip:
            assert g is image_t, (tag, k)       # the identity view is the input, not a copy
        else:
            assert g.data_ptr() != image_t.data_ptr()
        msg = C.same_bits(g.cpu().numpy(), v)
        assert msg is None, (tag, k, (scale, flip), msg)


# ------------------------------------------------------------------------------------------ the ops against the definition
@pytest.mark.parametrize("name", list(C.VIEW_SETS))
@pytest.mark.parametrize("shape", C.GPU_SHAPES)
def test_ops_are_the_definition(shape, name):
    from fosvos_hip import ops
    n, h, w = shape
    views = C.VIEW_SETS[name]
    seed = zlib.crc32(repr((shape, name)).encode()) & 0xFFFF
    x = C.image(n, h, w, seed)
    image_t = dev(x)
    check_views(ops.ensemble_views(image_t, views), image_t, x, views, (shape, name))
    assert np.array_equal(image_t.cpu().numpy(), x)
    maps = C.logit_maps(n, h, w, views, seed)
    maps_t = [dev(m) for m in maps]
    got = ops.ensemble_merge(maps_t, views, (h, w))
    assert tuple(got.shape) == (n, 1, h, w) and got.dtype == F32
    msg = C.same_bits(got.cpu().numpy(), TE.merge(maps, views, h, w))
    assert msg is None, (shape, name, msg)
    for m, t in zip(maps, maps_t):
        assert np.array_equal(t.cpu().numpy(), m)


def test_ops_write_into_the_callers_tensors():
    from fosvos_hip import ops
    n, h, w = 3, 33, 67
    x = C.image(n, h, w, 11)
    image_t = dev(x)
    out = [None if (s, f) == (1.0, F) else torch.full((n, 3) + TE.view_sizes(h, w, s), float("nan"), device=DEV) for s, f in C.EIGHT]
    got = ops.ensemble_views(image_t, C.EIGHT, out=out)
    assert all(g is o for g, o in zip(got[1:], out[1:])) and got[0] is image_t
    check_views(got, image_t, x, C.EIGHT, "out=")
    maps = C.logit_maps(n, h, w, C.EIGHT, 11)
    into = torch.full((n, 1, h, w), float("nan"), device=DEV)
    assert ops.ensemble_merge([dev(m) for m in maps], C.EIGHT, (h, w), out=into) is into
    assert C.same_bits(into.cpu().numpy(), TE.merge(maps, C.EIGHT, h, w)) is None


@pytest.mark.parametrize("shape", [(1, 13, 37), (2, 16, 64)])
def test_ops_on_tensors_one_float_past_a_16_byte_boundary(shape):
    from fosvos_hip import ops
    n, h, w = shape
    x = C.image(n, h, w, 12)
    image_t = carved(x.shape, x)
    out = [None if (s, f) == (1.0, F) else carved((n, 3) + TE.view_sizes(h, w, s)) for s, f in C.EIGHT]
    check_views(ops.ensemble_views(image_t, C.EIGHT, out=out), image_t, x, C.EIGHT, "carved")
    maps = C.logit_maps(n, h, w, C.EIGHT, 12)
    got = ops.ensemble_merge([carved(m.shape, m) for m in maps], C.EIGHT, (h, w), out=carved((n, 1, h, w)))
    assert C.same_bits(got.cpu().numpy(), TE.merge(maps, C.EIGHT, h, w)) is None


@pytest.mark.parametrize("shape", [(2, 5, 7), (1, 13, 37), (1, 48, 80)])
def test_merge_of_non_finite_values_and_signed_zeros(shape):
    """NaN, +inf, -inf and -0.0 in every map, and a lone map of -0.0: the rule of tests/test_ensemble_cases.same_bits."""
    from fosvos_hip import ops
    n, h, w = shape
    maps = C.with_specials(C.logit_maps(n, h, w, C.EIGHT, 13), 13)
    want = TE.merge(maps, C.EIGHT, h, w)
    got = ops.ensemble_merge([dev(m) for m in maps], C.EIGHT, (h, w)).cpu().numpy()
    print("non-finite %s: %d NaN, %d inf expected; %d NaNs differ in their bits" % (
        shape, int(np.isnan(want).sum()), int(np.isinf(want).sum()), C.nan_bits_that_differ(got, want)))
    assert np.isnan(want).any() and np.isinf(want).any()
    msg = C.same_bits(got, want)
    assert msg is None, msg
    for views in ([(1.0, F)], [(1.0, T)]):
        zeros = np.full((n, 1, h, w), -0.0, dtype=np.float32)
        lone = ops.ensemble_merge([dev(zeros)], views, (h, w)).cpu().numpy()
        assert (C.bits(lone) == 0x80000000).all()
    plus = ops.ensemble_merge([dev(zeros), dev(-zeros)], C.VIEW_SETS["flip"], (h, w)).cpu().numpy()
    assert (C.bits(plus) == 0).all()


# ------------------------------------------------------------------------------------------ islands
def _table(isl, names, views, h, w):
    from fosvos_hip import EnsembleView
    table = (EnsembleView * len(names))()
    for entry, name, (scale, flip) in zip(table, names, views):
        entry.data = isl.ptr(name)
        entry.h, entry.w = TE.view_sizes(h, w, scale)
        entry.flip = int(flip)
    return table


def test_both_entries_touch_nothing_outside_their_operands():
    from fosvos_hip import check, lib
    L = lib()
    n, h, w = 2, 13, 37
    stream = torch.cuda.current_stream(0).cuda_stream
    x = C.image(n, h, w, 14)
    made = C.EIGHT[1:]                         # the identity view is not produced
    want = TE.make_views(x, made)
    names = ["view%d" % k for k in range(len(made))]
    operands = [I.inp("image", torch.from_numpy(x), is_map=False, offset=4)]
    operands += [I.out(name, v.shape, F32, is_map=False, offset=4 * (k % 4)) for k, (name, v) in enumerate(zip(names, want))]

    def views_call(isl):
        check(L.fosvos_ensemble_views(isl.ptr("image"), n, h, w, _table(isl, names, made, h, w), len(made), 0, stream),
              "ensemble_views")

    rep = I.Report("ensemble 2x13x37, eight views")
    rep.add(I.run_case("views", operands, views_call, {name: torch.from_numpy(v) for name, v in zip(names, want)}, device=DEV,
                       seed=1))
    maps = C.logit_maps(n, h, w, C.EIGHT, 14)
    names = ["map%d" % k for k in range(8)]
    operands = [I.inp(name, torch.from_numpy(m), is_map=False, offset=4 * ((k + 1) % 4)) for k, (name, m) in enumerate(zip(names, maps))]
    operands.append(I.out("out", (n, 1, h, w), F32, is_map=False, offset=12))

    def merge_call(isl):
        check(L.fosvos_ensemble_merge(_table(isl, names, C.EIGHT, h, w), 8, n, h, w, isl.ptr("out"), 0, stream), "ensemble_merge")

    rep.add(I.run_case("merge", operands, merge_call, {"out": torch.from_numpy(TE.merge(maps, C.EIGHT, h, w))}, device=DEV, seed=2))
    rep.done()


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


def fault_rows():
    from fosvos_hip import ops
    n, h, w = 2, 12, 20
    views = [(1.0, F), (1.0, T), (0.5, T)]
    image = dev(C.image(n, h, w, 15))
    maps = [dev(m) for m in C.logit_maps(n, h, w, views, 15)]
    new = lambda shape, dtype=F32: torch.empty(shape, dtype=dtype, device=DEV)  # noqa: E731
    ev, em = "ensemble_views", "ensemble_merge"
    scale_msg = "a view's scale must be a finite number in [0.25, 4], got"
    wide = new((1, 3, 4, 4096))
    rows = [
        ("views image cpu", lambda: ops.ensemble_views(image.cpu(), views), RuntimeError, f"{ev} image: {NO_CPU}"),
        ("views image dtype", lambda: ops.ensemble_views(image.double(), views), ValueError,
         f"{ev} image: expected torch.float32, got torch.float64"),
        ("views image strided", lambda: ops.ensemble_views(strided(image), views), ValueError, f"{ev} image: tensor must be contiguous"),
        ("views image shape", lambda: ops.ensemble_views(image[:, :1].contiguous(), views), ValueError,
         f"{ev}: image must be a non-empty [N,3,H,W], got {(n, 1, h, w)}"),
        ("views image empty", lambda: ops.ensemble_views(new((0, 3, h, w)), views), ValueError,
         f"{ev}: image must be a non-empty [N,3,H,W], got {(0, 3, h, w)}"),
        ("views none", lambda: ops.ensemble_views(image, []), ValueError, f"{ev}: 0 views, outside [1, 8]"),
        ("views nine", lambda: ops.ensemble_views(image, [(1.0, T)] * 9), ValueError, f"{ev}: 9 views, outside [1, 8]"),
        ("views scale high", lambda: ops.ensemble_views(image, [(5.0, F)]), ValueError, f"{ev}: {scale_msg} 5.0"),
        ("views scale low", lambda: ops.ensemble_views(image, [(0.2, F)]), ValueError, f"{ev}: {scale_msg} 0.2"),
        ("views scale bool", lambda: ops.ensemble_views(image, [(True, F)]), ValueError, f"{ev}: {scale_msg} True"),
        ("views flip int", lambda: ops.ensemble_views(image, [(1.0, 1)]), ValueError, f"{ev}: a view's flip must be a bool, got 1"),
        ("views no pair", lambda: ops.ensemble_views(image, [1.0]), ValueError, f"{ev}: a view must be (scale, flip), got 1.0"),
        ("views side", lambda: ops.ensemble_views(wide, [(4.0, F)]), ValueError,
         f"{ev}: the view of scale 4.0 is (16, 16384), a side above 8192"),
        ("views out count", lambda: ops.ensemble_views(image, views, out=[None, None]), ValueError,
         f"{ev}: out must hold one entry per view (3), got 2"),
        ("views out identity", lambda: ops.ensemble_views(image, views, out=[new((n, 3, h, w)), None, None]), ValueError,
         f"{ev}: out[0] must be None: view 0 is the image itself"),
        ("views out shape", lambda: ops.ensemble_views(image, views, out=[None, None, new((n, 3, 6, 11))]), ValueError,
         f"{ev}: out[2] must be {(n, 3, 6, 10)}, got {(n, 3, 6, 11)}"),
        ("views out dtype", lambda: ops.ensemble_views(image, views, out=[None, new((n, 3, h, w), F64), None]), ValueError,
         f"{ev} out[1]: expected torch.float32, got torch.float64"),
        ("views out cpu", lambda: ops.ensemble_views(image, views, out=[None, torch.empty((n, 3, h, w)), None]), RuntimeError,
         f"{ev} out[1]: {NO_CPU}"),
        ("views out strided", lambda: ops.ensemble_views(image, views, out=[None, strided(new((n, 3, h, w))), None]), ValueError,
         f"{ev} out[1]: tensor must be contiguous"),
        ("views out is the image", lambda: ops.ensemble_views(image, views, out=[None, image, None]), ValueError,
         f"{ev}: out[1] must not overlap the image or another view"),
        ("views out twice", lambda t=new((n, 3, h, w)): ops.ensemble_views(image, [(1.0, T), (1.0, T)], out=[t, t]), ValueError,
         f"{ev}: out[1] must not overlap the image or another view"),
        ("merge size int", lambda: ops.ensemble_merge(maps, views, 5), ValueError, f"{em}: size must be a pair (H, W), got 5"),
        ("merge size zero", lambda: ops.ensemble_merge(maps, views, (0, w)), ValueError,
         f"{em}: size must be a pair of positive ints, got {(0, w)}"),
        ("merge none", lambda: ops.ensemble_merge([], [], (h, w)), ValueError, f"{em}: 0 views, outside [1, 8]"),
        ("merge nine", lambda: ops.ensemble_merge(maps[:1] * 9, [(1.0, F)] * 9, (h, w)), ValueError, f"{em}: 9 views, outside [1, 8]"),
        ("merge scale", lambda: ops.ensemble_merge(maps[:1], [(4.5, F)], (h, w)), ValueError, f"{em}: {scale_msg} 4.5"),
        ("merge side", lambda: ops.ensemble_merge(maps[:1], [(1.0, F)], (4, 8193)), ValueError,
         f"{em}: the view of scale 1.0 is (4, 8193), a side above 8192"),
        ("merge count", lambda: ops.ensemble_merge(maps[:2], views, (h, w)), ValueError, f"{em}: 2 logit maps for 3 views"),
        ("merge map cpu", lambda: ops.ensemble_merge([maps[0], maps[1].cpu(), maps[2]], views, (h, w)), RuntimeError,
         f"{em} logits: {NO_CPU}"),
        ("merge map dtype", lambda: ops.ensemble_merge([maps[0].double(), maps[1], maps[2]], views, (h, w)), ValueError,
         f"{em} logits: expected torch.float32, got torch.float64"),
        ("merge map strided", lambda: ops.ensemble_merge([maps[0], maps[1], strided(maps[2])], views, (h, w)), ValueError,
         f"{em} logits: tensor must be contiguous"),
        ("merge first map", lambda: ops.ensemble_merge([new((n, 2, h, w)), maps[1], maps[2]], views, (h, w)), ValueError,
         f"{em}: logits must be a non-empty [N,1,H,W], got {(n, 2, h, w)}"),
        ("merge map of a view", lambda: ops.ensemble_merge([maps[0], maps[1], new((n, 1, 6, 11))], views, (h, w)), ValueError,
         f"{em}: the map of view 2 (0.5, True) must be {(n, 1, 6, 10)}, got {(n, 1, 6, 11)}"),
        ("merge map of another size", lambda: ops.ensemble_merge(maps, views, (h, w + 1)), ValueError,
         f"{em}: the map of view 0 (1.0, False) must be {(n, 1, h, w + 1)}, got {(n, 1, h, w)}"),
        ("merge out shape", lambda: ops.ensemble_merge(maps, views, (h, w), out=new((n, h, w))), ValueError,
         f"{em}: out must be {(n, 1, h, w)}, got {(n, h, w)}"),
        ("merge out dtype", lambda: ops.ensemble_merge(maps, views, (h, w), out=new((n, 1, h, w), F64)), ValueError,
         f"{em} out: expected torch.float32, got torch.float64"),
        ("merge out cpu", lambda: ops.ensemble_merge(maps, views, (h, w), out=torch.empty((n, 1, h, w))), RuntimeError,
         f"{em} out: {NO_CPU}"),
        ("merge out is a map", lambda: ops.ensemble_merge(maps, views, (h, w), out=maps[1]), ValueError,
         f"{em}: out must not overlap a logit map"),
    ]
    return rows


def test_a_fault_raises_before_any_launch():
    missed = []
    for label, call, error, message in fault_rows():
        with recording() as rec:
            try:
                call()
                got = "no exception"
            except Exception as e:  # noqa: BLE001  (the row names the one it expects)
                got = (type(e), str(e))
        if got != (error, message) or rec.launches:
            missed.append(f"{label}: expected {(error, message)}, got {got}, launches {rec.launches}")
    assert not missed, "\n".join(missed)


def test_good_calls_launch_once_and_the_identity_alone_launches_nothing():
    from fosvos_hip import ops
    n, h, w = 2, 12, 20
    image = dev(C.image(n, h, w, 16))
    with recording() as rec:
        assert ops.ensemble_views(image, [(1.0, F)])[0] is image
        assert rec.launches == []
        ops.ensemble_views(image, C.EIGHT)
        assert rec.launches == ["fosvos_ensemble_views"]
        ops.ensemble_merge([dev(m) for m in C.logit_maps(n, h, w, C.EIGHT, 16)], C.EIGHT, (h, w))
        assert rec.launches == ["fosvos_ensemble_views", "fosvos_ensemble_merge"]


def test_the_c_entries_refuse_their_faults_with_a_code_and_a_message():
    import fosvos_hip
    from fosvos_hip import EnsembleView
    L = fosvos_hip.lib()
    E_SHAPE, E_ARG = -1, -2
    n, h, w = 1, 4, 8
    image, view, out = dev(C.image(n, h, w, 17)), torch.empty((n, 3, h, w), device=DEV), torch.empty((n, 1, h, w), device=DEV)

    def table(count=1, data=view.data_ptr(), hs=h, ws=w):
        t = (EnsembleView * max(count, 1))()
        for e in t:
            e.data, e.h, e.w, e.flip = data, hs, ws, 1
        return t

    cases = [
        (lambda: L.fosvos_ensemble_views(None, n, h, w, table(), 1, 0, None), E_ARG, "ensemble_views: null pointer"),
        (lambda: L.fosvos_ensemble_views(image.data_ptr(), n, h, w, None, 1, 0, None), E_ARG, "ensemble_views: null pointer"),
        (lambda: L.fosvos_ensemble_views(image.data_ptr(), n, h, w, table(data=None), 1, 0, None), E_ARG, "ensemble_views: null view 0"),
        (lambda: L.fosvos_ensemble_views(image.data_ptr(), n, h, w, table(), 0, 0, None), E_ARG, "ensemble_views: V=0 outside [1, 8]"),
        (lambda: L.fosvos_ensemble_views(image.data_ptr(), n, h, w, table(9), 9, 0, None), E_ARG, "ensemble_views: V=9 outside [1, 8]"),
        (lambda: L.fosvos_ensemble_views(image.data_ptr(), n, h, w, table(ws=8193), 1, 0, None), E_SHAPE,
         "ensemble_views: view 0 is 4 x 8193, sides outside 1..8192"),
        (lambda: L.fosvos_ensemble_views(image.data_ptr(), n, h, w, table(hs=0), 1, 0, None), E_SHAPE,
         "ensemble_views: view 0 is 0 x 8, sides outside 1..8192"),
        (lambda: L.fosvos_ensemble_views(image.data_ptr(), n, 8193, w, table(), 1, 0, None), E_SHAPE,
         "ensemble_views: the frame is 8193 x 8, sides outside 1..8192"),
        (lambda: L.fosvos_ensemble_views(image.data_ptr(), 0, h, w, table(), 1, 0, None), E_SHAPE, "ensemble_views: N=0 outside 1..65535"),
        (lambda: L.fosvos_ensemble_views(image.data_ptr(), 65536, h, w, table(), 1, 0, None), E_SHAPE,
         "ensemble_views: N=65536 outside 1..65535"),
        (lambda: L.fosvos_ensemble_merge(table(), 1, n, h, w, None, 0, None), E_ARG, "ensemble_merge: null pointer"),
        (lambda: L.fosvos_ensemble_merge(None, 1, n, h, w, out.data_ptr(), 0, None), E_ARG, "ensemble_merge: null pointer"),
        (lambda: L.fosvos_ensemble_merge(table(data=None), 1, n, h, w, out.data_ptr(), 0, None), E_ARG, "ensemble_merge: null view 0"),
        (lambda: L.fosvos_ensemble_merge(table(), 0, n, h, w, out.data_ptr(), 0, None), E_ARG, "ensemble_merge: V=0 outside [1, 8]"),
        (lambda: L.fosvos_ensemble_merge(table(9), 9, n, h, w, out.data_ptr(), 0, None), E_ARG, "ensemble_merge: V=9 outside [1, 8]"),
        (lambda: L.fosvos_ensemble_merge(table(hs=8193), 1, n, h, w, out.data_ptr(), 0, None), E_SHAPE,
         "ensemble_merge: view 0 is 8193 x 8, sides outside 1..8192"),
        (lambda: L.fosvos_ensemble_merge(table(), 1, n, h, 0, out.data_ptr(), 0, None), E_SHAPE,
         "ensemble_merge: the frame is 4 x 0, sides outside 1..8192"),
        (lambda: L.fosvos_ensemble_merge(table(), 1, 65536, h, w, out.data_ptr(), 0, None), E_SHAPE,
         "ensemble_merge: N=65536 outside 1..65535"),
    ]
    torch.cuda.synchronize()
    with fosvos_hip.LaunchProfile(0) as prof:
        got = [(call(), L.fosvos_last_error().decode()) for call, _, _ in cases]
    assert got == [(code, message) for _, code, message in cases]
    assert prof.records == {}
    assert ctypes.sizeof(EnsembleView) == 24


# ------------------------------------------------------------------------------------------ the passes on the real net
SIZE = PC.SIZE
SIX = TE.views(True, (0.75, 1.0, 1.25))


def six():
    from fosvos_hip.options import EnsembleOptions
    return EnsembleOptions(flip=True, scales=(0.75, 1.0, 1.25))


class Recorder(PC.Recorder):
    """The recorder of tests/test_gpu_test_pass_calls.py with the two ensemble ops logged as well."""

    @contextlib.contextmanager
    def active(self, monkeypatch):
        from fosvos_hip import ops
        with super().active(monkeypatch):
            with monkeypatch.context() as m:
                for name in ("ensemble_views", "ensemble_merge"):
                    m.setattr(ops, name, self._op(name, getattr(ops, name)))
                yield self


def by_definition(provider, views):
    """The provider's net behind the numpy definition: what a pass with ``ensemble`` must equal."""
    return C.Provider(C.EnsembleByDefinition(provider.network, views, device=DEV))


@pytest.mark.parametrize("clean", [False, True])
def test_fast_with_an_ensemble_writes_the_definitions_files(clean, tmp_path):
    """4 frames of 48x80 (views of 36x60 and 60x100) in groups of 3 and 1, two frames a forward call - which keeps each
    frame's arithmetic, so the comparison is byte for byte."""
    from fosvos_hip.options import CleanOptions
    assert [TE.view_sizes(*SIZE, s) for s in (0.75, 1.25)] == [(36, 60), (60, 100)]
    kw = {"clean": CleanOptions(largest=True)} if clean else {}
    prov = PC.Provider(PC.Recorder())
    loader = PC.blob_loader(4)
    score = experiment_helper.test_fast(prov, loader, tmp_path / "ensemble", loader.dataset.annotation, group=3,
                                        forward_batch=2, seq_name="blob", ensemble=six(), **kw)
    assert score["ensemble"] == {"flip": True, "scales": [0.75, 1.0, 1.25]} == experiment_helper.last_fast["ensemble"]
    assert experiment_helper.last_fast["group_sizes"] == [3, 1]
    loader = PC.blob_loader(4)
    want = experiment_helper.test_fast(by_definition(prov, SIX), loader, tmp_path / "definition", loader.dataset.annotation,
                                       group=3, forward_batch=2, seq_name="blob", **kw)
    files = C.files_of(tmp_path / "ensemble")
    assert sorted(files) == ["blob/%05d.png" % k for k in range(4)]
    assert files == C.files_of(tmp_path / "definition")
    for key in ("counts", "J", "F", "J_stats", "F_stats", "J&F", "fnames", "scored"):
        assert score[key] == want[key], key
    assert "ensemble" not in want


def test_objects_with_an_ensemble_writes_the_definitions_files(tmp_path):
    from dataloaders.synthetic import SyntheticObjectsSequence
    from torch.utils.data import DataLoader
    rec = PC.Recorder()
    providers = [PC.Provider(rec, seed=2, name="forward net 1"), PC.Provider(rec, seed=3, name="forward net 2")]
    data = SyntheticObjectsSequence("blobs", SIZE[0], SIZE[1], n_frames=4, n_objects=2)

    def loader():
        return DataLoader(data, batch_size=1, shuffle=False, num_workers=0)

    score = experiment_helper.test_objects(providers, loader(), tmp_path / "ensemble", data.annotation, group=3, forward_batch=2,
                                           seq_name="blobs", ensemble=six())
    want = experiment_helper.test_objects([by_definition(p, SIX) for p in providers], loader(), tmp_path / "definition",
                                          data.annotation, group=3, forward_batch=2, seq_name="blobs")
    files = C.files_of(tmp_path / "ensemble")
    assert sorted(files) == ["blobs/%05d.png" % k for k in range(4)] and files == C.files_of(tmp_path / "definition")
    assert score["ensemble"] == six().as_dict() and "ensemble" not in want
    assert [o["counts"] for o in score["objects"]] == [o["counts"] for o in want["objects"]]
    assert score["J&F"] == want["J&F"] and score["n_objects"] == 2


def forwards(name, n, forward_batch, n_views=6):
    """The forward calls of one net for one group: view by view, ``forward_batch`` frames a call."""
    return [(name, min(forward_batch, n - k)) for _ in range(n_views) for k in range(0, n, forward_batch)]


def test_fast_call_order(tmp_path, monkeypatch):
    """5 frames in groups of 3 and 2, two frames a forward call.  Per group: ``ensemble_views`` once, the forward calls view
    by view, ``ensemble_merge`` once, then the sequence as without an ensemble - and no host wait beyond that one's."""
    rec = Recorder()
    prov = PC.Provider(rec)
    loader = PC.blob_loader(5)
    with rec.active(monkeypatch):
        experiment_helper.test_fast(prov, loader, tmp_path / "a", loader.dataset.annotation, group=3, forward_batch=2,
                                    seq_name="blob", ensemble=six())
    expected = []
    for g, n in enumerate([3, 2]):
        expected += [("ensemble_views", ())] + forwards("forward", n, 2) + [("ensemble_merge", ())]
        expected += [("jf_counts", ("out",)), ("prob_bytes", ()), ("png_encode", ("out", "lengths"))]
        expected += [PC.EVENT_WAIT] if g > 0 else []
    expected += [PC.EVENT_WAIT, PC.READ_BACK]
    assert rec.log == expected
    # without an ensemble no ensemble op is called: the sequence tests/test_gpu_test_pass_calls.py pins
    rec = Recorder()
    prov = PC.Provider(rec)
    loader = PC.blob_loader(5)
    with rec.active(monkeypatch):
        experiment_helper.test_fast(prov, loader, tmp_path / "b", loader.dataset.annotation, group=2, seq_name="blob")
    assert rec.log == PC.fast_expected([2, 2, 1], True)


def test_objects_call_order(tmp_path, monkeypatch):
    """2 nets, 3 frames in groups of 2 and 1: the views are made once a group; each net forwards them and has its answers
    merged before the label merge."""
    from dataloaders.synthetic import SyntheticObjectsSequence
    from torch.utils.data import DataLoader
    data = SyntheticObjectsSequence("blobs", SIZE[0], SIZE[1], n_frames=3, n_objects=2)

    def run(where, **kw):
        rec = Recorder()
        providers = [PC.Provider(rec, seed=2, name="forward net 1"), PC.Provider(rec, seed=3, name="forward net 2")]
        with rec.active(monkeypatch):
            experiment_helper.test_objects(providers, DataLoader(data, batch_size=1, shuffle=False, num_workers=0),
                                           tmp_path / where, data.annotation, group=2, seq_name="blobs", **kw)
        return rec.log

    tail = [("merge_objects", ()), ("jf_counts_labels", ("out",)), ("png_encode_indexed", ("out", "lengths"))]
    expected, plain = [], []
    for g, n in enumerate([2, 1]):
        expected += [("ensemble_views", ())]
        for name in ("forward net 1", "forward net 2"):
            expected += forwards(name, n, 2) + [("ensemble_merge", ())]
        expected += tail + ([PC.EVENT_WAIT] if g > 0 else [])
        plain += [("forward net 1", n), ("forward net 2", n)] + tail + ([PC.EVENT_WAIT] if g > 0 else [])
    assert run("a", ensemble=six()) == expected + [PC.EVENT_WAIT, PC.READ_BACK]
    assert run("b") == plain + [PC.EVENT_WAIT, PC.READ_BACK]
