"""The test-time ensemble without a GPU: the numpy definition the HIP kernels are tested against (util/test_ensemble.py), its
exact identities, the registration of the merged map, how non-finite values travel, ``EnsembleOptions``, the parser's flags
and the host path of ``test_fast(ensemble=)`` and ``test_objects(ensemble=)``."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_ensemble_cases as C  # noqa: E402
from fosvos_hip import limits  # noqa: E402
from fosvos_hip.options import CleanOptions, EnsembleOptions  # noqa: E402
from util import args_helper, experiment_helper, frame_resample, io_helper, test_ensemble as TE  # noqa: E402

F, T = False, True


# ------------------------------------------------------------------------------------------ views
@pytest.mark.parametrize("frame,scale,want", C.VIEW_SIZES)
def test_view_sizes(frame, scale, want):
    assert TE.view_sizes(frame[0], frame[1], scale) == want


def test_views_lists_each_scale_and_then_its_mirror():
    assert TE.views(False, (1.0,)) == [(1.0, F)]
    assert TE.views(True, (1.0,)) == [(1.0, F), (1.0, T)]
    assert TE.views(True, (0.5, 1.0, 2.0)) == [(0.5, F), (0.5, T), (1.0, F), (1.0, T), (2.0, F), (2.0, T)]
    assert TE.views(False, [1.25, 0.75]) == [(1.25, F), (0.75, F)]
    assert (TE.MAX_VIEWS, TE.SCALE_RANGE, TE.MAX_SIDE) == (8, (0.25, 4.0), 8192)


def test_definition_reuses_the_taps_of_frame_resample():
    assert TE.taps is frame_resample.taps


@pytest.mark.parametrize("n_src", [1, 2, 5, 7, 13, 37, 67])
def test_taps_serve_both_directions(n_src):
    """Scales 0.25 .. 4 at seven sizes: indices in range, weights not negative, each pair sums to ``2 n_dst``."""
    for scale in C.SCALES + [1.0]:
        n_dst = TE.view_sizes(n_src, n_src, scale)[0]
        i0, i1, w0, w1 = frame_resample.taps(n_src, n_dst)
        assert i0.min() >= 0 and i1.max() <= n_src - 1 and ((i1 == i0) | (i1 == i0 + 1)).all()
        assert (w0 > 0).all() and (w1 >= 0).all() and np.array_equal(w0 + w1, np.full(n_dst, 2.0 * n_dst))


def test_check_views_bounds():
    for bad in ([], [(1.0, F)] * 9, [(0.2, F)], [(4.5, F)], [(True, F)], [(1.0, 1)], [1.0], [(float("nan"), F)]):
        with pytest.raises(ValueError):
            TE.check_views(bad, 8, 8)
    with pytest.raises(ValueError):
        TE.check_views([(4.0, F)], 4096, 8)      # a side of 16384
    assert TE.check_views([(2, T)], 8, 8) == [(2.0, True)]


# ------------------------------------------------------------------------------------------ exact identities
@pytest.mark.parametrize("shape", C.SHAPES)
def test_same_size_resample_is_the_input(shape):
    a = C.image(1, *shape, seed=1)[0, 0]
    assert C.same_bits(TE.resample(a, *shape).astype(np.float32), a) is None


@pytest.mark.parametrize("shape", C.SHAPES)
def test_resample_commutes_with_the_mirror(shape):
    a = C.image(1, *shape, seed=2)[0, 0]
    for scale in C.SCALES:
        ho, wo = TE.view_sizes(shape[0], shape[1], scale)
        assert np.array_equal(TE.resample(np.ascontiguousarray(a[:, ::-1]), ho, wo), TE.resample(a, ho, wo)[:, ::-1])


def test_a_constant_map_stays_that_constant():
    a = np.full((13, 37), 1.7, dtype=np.float32)
    for scale in (0.5, 0.75, 1.25, 2.0):
        out = TE.resample(a, *TE.view_sizes(13, 37, scale)).astype(np.float32)
        assert (C.bits(out) == C.bits(a)[0, 0]).all(), scale


@pytest.mark.parametrize("shape", C.SHAPES)
def test_merge_of_copies_is_the_map(shape):
    a = C.image(2, *shape, seed=3, channels=1)
    for v in range(1, 9):
        assert C.same_bits(TE.merge([a] * v, [(1.0, F)] * v, *shape), a) is None, v


def test_make_views_same_size_views_are_copies():
    x = C.image(2, 5, 7, seed=4)
    plain, mirrored = TE.make_views(x, [(1.0, F), (1.0, T)])
    assert np.array_equal(plain, x) and plain is not x and not np.shares_memory(plain, x)
    assert np.array_equal(mirrored, x[..., ::-1]) and mirrored.flags["C_CONTIGUOUS"]
    small, = TE.make_views(x, [(0.5, T)])
    assert small.shape == (2, 3, 3, 4) and small.dtype == np.float32
    assert np.array_equal(small[1, 2], TE.resample(np.ascontiguousarray(x[1, 2, :, ::-1]), 3, 4).astype(np.float32))


def test_merge_order_and_division():
    """``acc = u_0``, ``acc += u_k`` in list order in float64, one division by V, one rounding."""
    h, w = 5, 7
    views = [(1.0, F), (0.5, T), (2.0, F)]
    maps = C.logit_maps(2, h, w, views, seed=5)
    acc = maps[0].astype(np.float64)
    acc = acc + np.stack([TE.resample(maps[1][i, 0], h, w)[None] for i in range(2)])[..., ::-1]
    acc = acc + np.stack([TE.resample(maps[2][i, 0], h, w)[None] for i in range(2)])
    assert C.same_bits(TE.merge(maps, views, h, w), (acc / np.float64(3)).astype(np.float32)) is None
    with pytest.raises(ValueError):
        TE.merge(maps[:2], views, h, w)
    with pytest.raises(ValueError):
        TE.merge([maps[0], maps[2], maps[1]], views, h, w)
    lone = np.full((1, 1, h, w), -0.0, dtype=np.float32)
    assert (C.bits(TE.merge([lone], [(1.0, F)], h, w)) == 0x80000000).all()


# ------------------------------------------------------------------------------------------ registration
@pytest.mark.parametrize("shape", [(13, 37), (48, 80)])
def test_the_merged_map_lies_on_the_frames_grid(shape):
    """The stub net returns channel 0 of what it sees; the input is ``x + 3 y``.  The bounds: a bilinear view of a plane is
    the plane itself between the outermost sample centres, so inside the merged map is the input up to rounding (< 1e-3 two
    pixels in); at the border the clamped taps of a view move a value by at most half a source step per axis and view, (1 + 3)
    / 2 at scale 0.5, and the mean over eight views of which two are exact stays below 1.  A view that is not mirrored back
    misses by up to W - 1."""
    h, w = shape
    x = C.ramp(h, w)
    maps = [v[:, :1].copy() for v in TE.make_views(x, C.EIGHT)]
    err = np.abs(TE.merge(maps, C.EIGHT, h, w)[0, 0].astype(np.float64) - x[0, 0])
    print("registration %s: max error %.4f overall, %.6f two pixels inside" % (shape, err.max(), err[2:-2, 2:-2].max()))
    assert err.max() < 1.0 and err[2:-2, 2:-2].max() < 1e-3
    unflipped = [(s, F) for s, _ in C.EIGHT]   # the maps of the mirrored views taken as if they were not
    miss = np.abs(TE.merge(maps, unflipped, h, w)[0, 0].astype(np.float64) - x[0, 0])
    assert miss.max() > 1.0


# ------------------------------------------------------------------------------------------ non-finite values
def _touched(h, w, view, hs, ws, y, x):
    """The output pixels [h,w] one of whose four taps in a map [hs,ws] of ``view`` is pixel (y, x), and those among them that
    touch it through a tap of weight 0 as well."""
    y0, y1, wy0, wy1 = frame_resample.taps(hs, h)
    x0, x1, wx0, wx1 = frame_resample.taps(ws, w)
    rows, cols = (y0 == y) | (y1 == y), (x0 == x) | (x1 == x)
    zero_y = ((y0 == y) & (wy0 == 0)) | ((y1 == y) & (wy1 == 0))
    zero_x = ((x0 == x) & (wx0 == 0)) | ((x1 == x) & (wx1 == 0))
    hit = rows[:, None] & cols[None, :]
    zero = hit & (zero_y[:, None] | zero_x[None, :])
    return (hit[:, ::-1], zero[:, ::-1]) if view[1] else (hit, zero)


@pytest.mark.parametrize("shape", [(5, 7), (13, 37)])
def test_a_nan_reaches_exactly_the_pixels_whose_taps_touch_it(shape):
    h, w = shape
    rng = np.random.default_rng(6)
    maps = C.logit_maps(1, h, w, C.EIGHT, seed=6)
    clean = TE.merge(maps, C.EIGHT, h, w)
    for k, view in enumerate(C.EIGHT):
        hs, ws = maps[k].shape[2:]
        y, x = int(rng.integers(0, hs)), int(rng.integers(0, ws))
        poisoned = [m.copy() for m in maps]
        poisoned[k][0, 0, y, x] = np.nan
        got = TE.merge(poisoned, C.EIGHT, h, w)
        if (hs, ws) == (h, w):
            hit = np.zeros((h, w), dtype=bool)
            hit[y, w - 1 - x if view[1] else x] = True
        else:
            hit, _ = _touched(h, w, view, hs, ws, y, x)
        assert hit.any() and np.array_equal(np.isnan(got[0, 0]), hit), (k, view)
        assert np.array_equal(C.bits(got)[0, 0][~hit], C.bits(clean)[0, 0][~hit]), (k, view)


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_an_inf_propagates(sign):
    """Through taps of positive weight an infinity arrives as itself; where one of the taps that touch it has the weight 0 (a
    clamped border, a sample that sits on a centre) it arrives as inf x 0, a NaN.  Everything else keeps its bits."""
    h, w = 13, 37
    maps = C.logit_maps(1, h, w, C.EIGHT, seed=7)
    clean = TE.merge(maps, C.EIGHT, h, w)
    value = np.float32(sign * np.inf)
    for k, view in enumerate(C.EIGHT):
        hs, ws = maps[k].shape[2:]
        poisoned = [m.copy() for m in maps]
        poisoned[k][0, 0, hs // 2, ws // 3] = value
        got = TE.merge(poisoned, C.EIGHT, h, w)[0, 0]
        if (hs, ws) == (h, w):
            x = ws // 3
            hit = np.zeros((h, w), dtype=bool)
            hit[hs // 2, w - 1 - x if view[1] else x] = True
            zero = np.zeros((h, w), dtype=bool)
        else:
            hit, zero = _touched(h, w, view, hs, ws, hs // 2, ws // 3)
        assert (C.bits(got[hit & ~zero]) == C.bits(value)).all() and (hit & ~zero).any()
        assert np.isnan(got[zero]).all()
        assert np.array_equal(C.bits(got)[~hit], C.bits(clean)[0, 0][~hit]), (k, view)


# ------------------------------------------------------------------------------------------ options and limits
def test_limits_equal_the_definitions():
    assert limits.ENSEMBLE_MAX_VIEWS == TE.MAX_VIEWS == 8
    assert limits.ENSEMBLE_SCALE_RANGE == TE.SCALE_RANGE == (0.25, 4.0)
    assert limits.MAX_FRAME_SIDE == TE.MAX_SIDE


def test_ensemble_options():
    o = EnsembleOptions(flip=True, scales=(0.75, 1, 1.25))
    assert o.views() == TE.views(True, (0.75, 1.0, 1.25)) and len(o.views()) == 6
    assert o.as_dict() == {"flip": True, "scales": [0.75, 1.0, 1.25]}
    assert EnsembleOptions(flip=True).views() == [(1.0, F), (1.0, T)]
    assert EnsembleOptions(scales=[0.5, 2.0]).scales == (0.5, 2.0)
    assert len(EnsembleOptions(flip=True, scales=(0.25, 0.5, 1.0, 4.0)).views()) == 8
    assert len(EnsembleOptions(scales=(0.25, 0.5, 0.75, 1.0, 1.25, 2.0, 3.0, 4.0)).views()) == 8
    with pytest.raises(Exception):
        o.flip = False
    for kw, message in (
            ({}, "EnsembleOptions: the frame as it is, once, is no ensemble: set flip or give further scales"),
            ({"scales": (1,)}, "EnsembleOptions: the frame as it is, once, is no ensemble: set flip or give further scales"),
            ({"scales": (0.5,)}, "EnsembleOptions: 1 views, outside [2, 8] (1 scales)"),
            ({"flip": True, "scales": (0.5, 0.75, 1.0, 1.25, 2.0)},
             "EnsembleOptions: 10 views, outside [2, 8] (5 scales, each also mirrored)"),
            ({"scales": tuple(0.25 + 0.25 * k for k in range(9))}, "EnsembleOptions: 9 views, outside [2, 8] (9 scales)"),
            ({"flip": 1}, "EnsembleOptions: flip must be a bool, got 1"),
            ({"flip": True, "scales": ()}, "EnsembleOptions: scales must be a non-empty tuple of numbers, got ()"),
            ({"flip": True, "scales": 1.0}, "EnsembleOptions: scales must be a non-empty tuple of numbers, got 1.0"),
            ({"scales": (0.2, 1.0)}, "EnsembleOptions: scales must be finite numbers in [0.25, 4], got 0.2"),
            ({"scales": (1.0, 4.5)}, "EnsembleOptions: scales must be finite numbers in [0.25, 4], got 4.5"),
            ({"scales": (1.0, float("nan"))}, "EnsembleOptions: scales must be finite numbers in [0.25, 4], got nan"),
            ({"scales": (1.0, True)}, "EnsembleOptions: scales must be finite numbers in [0.25, 4], got True"),
            ({"scales": (1.0, "2")}, "EnsembleOptions: scales must be finite numbers in [0.25, 4], got '2'"),
            ({"scales": (1.0, 0.5, 1)}, "EnsembleOptions: scales must be distinct, got (1.0, 0.5, 1)")):
        with pytest.raises(ValueError) as err:
            EnsembleOptions(**kw)
        assert str(err.value) == message


# ------------------------------------------------------------------------------------------ the parser
def test_ensemble_flags_combine():
    a = args_helper.parse_args(True, ["--fast-test", "--ensemble-flip"])
    assert a.ensemble == EnsembleOptions(flip=True)
    a = args_helper.parse_args(True, ["--fast-test", "--ensemble-scales", "0.75", "1", "1.25", "--ensemble-flip"])
    assert a.ensemble == EnsembleOptions(flip=True, scales=(0.75, 1.0, 1.25))
    a = args_helper.parse_args(True, ["--synthetic", "--multi-object", "--ensemble-scales", "0.5", "1"])
    assert a.ensemble == EnsembleOptions(scales=(0.5, 1.0)) and a.multi_object
    a = args_helper.parse_args(True, ["--fast-test", "--score", "--png-fitted", "--clean-largest", "--clean-min-area", "9",
                                      "--clean-temporal", "3", "--device-decode", "--ensemble-flip"])
    assert a.ensemble == EnsembleOptions(flip=True) and a.score and a.png_fitted and a.clean_largest and a.device_decode
    a = args_helper.parse_args(True, ["--multi-object", "--score", "--png-fitted", "--ensemble-flip"])
    assert a.ensemble == EnsembleOptions(flip=True)
    assert args_helper.parse_args(True, ["--fast-test"]).ensemble is None
    assert args_helper.parse_args(True, []).ensemble is None
    assert not hasattr(args_helper.parse_args(False, []), "ensemble")
    with pytest.raises(SystemExit):
        args_helper.parse_args(False, ["--ensemble-flip"])      # an online flag


WHO = "--ensemble-flip / --ensemble-scales "


@pytest.mark.parametrize("argv,message", [
    (["--ensemble-flip"], WHO + "average the logits of the device test pass: they need --fast-test or --multi-object"),
    (["--score", "--ensemble-scales", "0.5", "1"],
     WHO + "average the logits of the device test pass: they need --fast-test or --multi-object"),
    (["--adapt-steps", "1", "--ensemble-flip"],
     WHO + "average the logits of the device test pass: they need --fast-test or --multi-object"),
    (["--fast-test", "--adapt-steps", "1", "--ensemble-flip"],
     WHO + "average the answers of a frozen net; adaptation of an ensemble (--adapt-steps) is not built"),
    (["--fast-test", "--eval-speeds", "--ensemble-flip"],
     WHO + "belong to a PNG-writing test pass; --eval-speeds times one forward and writes nothing"),
    (["--fast-test", "--data-parallel", "--ensemble-flip"],
     WHO + "run every view on one device; --data-parallel spreads a training cycle over the ranks"),
    (["--fast-test", "--ensemble-scales", "1"],
     "--ensemble-*: the frame as it is, once, is no ensemble: set flip or give further scales"),
    (["--fast-test", "--ensemble-scales", "0.5"], "--ensemble-*: 1 views, outside [2, 8] (1 scales)"),
    (["--fast-test", "--ensemble-scales", "1", "5"], "--ensemble-*: scales must be finite numbers in [0.25, 4], got 5.0"),
    (["--fast-test", "--ensemble-scales", "1", "1.0"], "--ensemble-*: scales must be distinct, got (1.0, 1.0)"),
    (["--fast-test", "--ensemble-flip", "--ensemble-scales", "0.5", "0.75", "1", "1.25", "2"],
     "--ensemble-*: 10 views, outside [2, 8] (5 scales, each also mirrored)")])
def test_ensemble_flag_refusals_say_why(argv, message, capsys):
    with pytest.raises(SystemExit):
        args_helper.parse_args(True, argv)
    assert capsys.readouterr().err.rstrip().split("error: ", 1)[1] == message


# ------------------------------------------------------------------------------------------ the passes, host path
SIX = TE.views(True, (0.75, 1.0, 1.25))


def _view_calls(views, n_frames_of_call, h, w, channels=3):
    return [(n, channels) + TE.view_sizes(h, w, s) for s, _ in views for n in n_frames_of_call]


@pytest.mark.parametrize("clean", [None, CleanOptions(largest=True)])
def test_fast_with_an_ensemble_on_cpu_tensors(tmp_path, clean):
    """5 frames of 24x40 in groups of 3 and 2, two frames a forward call: the stub sees every view of a group in view order,
    and the files and the score are those of the pass without ``ensemble`` over a net that applies the definition itself."""
    h, w = 24, 40
    opts = EnsembleOptions(flip=True, scales=(0.75, 1.0, 1.25))
    kw = {} if clean is None else {"clean": clean}

    def loader():
        return io_helper.get_data_loader_test(None, 1, "blob", synthetic=(h, w), n_frames=5)

    stub = C.StubNet()
    data = loader()
    score = experiment_helper.test_fast(C.Provider(stub), data, tmp_path / "ensemble", data.dataset.annotation, group=3,
                                        seq_name="blob", ensemble=opts, **kw)
    assert stub.calls == _view_calls(SIX, (2, 1), h, w) + _view_calls(SIX, (2,), h, w)
    assert score["ensemble"] == opts.as_dict() == experiment_helper.last_fast["ensemble"]
    assert experiment_helper.last_fast["group_sizes"] == [3, 2]
    inner = C.StubNet()
    data = loader()
    want = experiment_helper.test_fast(C.Provider(C.EnsembleByDefinition(inner, SIX)), data, tmp_path / "definition",
                                       data.dataset.annotation, group=3, seq_name="blob", **kw)
    assert "ensemble" not in want and "ensemble" not in experiment_helper.last_fast
    files = C.files_of(tmp_path / "ensemble")
    assert sorted(files) == ["blob/%05d.png" % k for k in range(5)] and files == C.files_of(tmp_path / "definition")
    for key in ("counts", "J", "F", "J_stats", "F_stats", "J&F", "fnames", "scored"):
        assert score[key] == want[key], key
    assert 0.0 < score["J_stats"]["mean"] <= 1.0
    # ... and they are not the files of the plain pass: the ensemble changes pixels
    data = loader()
    experiment_helper.test_fast(C.Provider(C.StubNet()), data, tmp_path / "plain", data.dataset.annotation, group=3,
                                seq_name="blob", **kw)
    assert C.files_of(tmp_path / "plain") != files


def test_objects_with_an_ensemble_on_cpu_tensors(tmp_path):
    """3 nets, 4 frames in groups of 3 and 1: the views are made once a group and every net sees them in view order."""
    from dataloaders.synthetic import SyntheticObjectsSequence
    from torch.utils.data import DataLoader
    h, w = 24, 40
    views = [(1.0, F), (1.0, T), (0.5, F), (0.5, T)]
    opts = EnsembleOptions(flip=True, scales=(1.0, 0.5))
    data = SyntheticObjectsSequence("blobs", h, w, n_frames=4, n_objects=3)

    def loader():
        return DataLoader(data, batch_size=1, shuffle=False, num_workers=0)

    made = []
    original = experiment_helper._ensemble_inputs

    def counted(inputs, ensemble):
        made.append(tuple(inputs.shape))
        return original(inputs, ensemble)

    stubs = [C.StubNet(channel=k, scale=0.125 + 0.05 * k) for k in range(3)]
    experiment_helper._ensemble_inputs = counted
    try:
        score = experiment_helper.test_objects([C.Provider(s) for s in stubs], loader(), tmp_path / "ensemble", data.annotation,
                                               group=3, seq_name="blobs", ensemble=opts)
    finally:
        experiment_helper._ensemble_inputs = original
    assert made == [(3, 3, h, w), (1, 3, h, w)]
    for s in stubs:
        assert s.calls == _view_calls(views, (2, 1), h, w) + _view_calls(views, (1,), h, w)
    assert score["ensemble"] == opts.as_dict() and score["n_objects"] == 3
    inner = [C.StubNet(channel=k, scale=0.125 + 0.05 * k) for k in range(3)]
    want = experiment_helper.test_objects([C.Provider(C.EnsembleByDefinition(s, views)) for s in inner], loader(),
                                          tmp_path / "definition", data.annotation, group=3, seq_name="blobs")
    assert "ensemble" not in want
    files = C.files_of(tmp_path / "ensemble")
    assert sorted(files) == ["blobs/%05d.png" % k for k in range(4)] and files == C.files_of(tmp_path / "definition")
    assert [o["counts"] for o in score["objects"]] == [o["counts"] for o in want["objects"]]
    assert score["J&F"] == want["J&F"]


def test_without_an_ensemble_the_helper_is_forward_logits():
    stub = C.StubNet()
    x = torch.from_numpy(C.image(3, 6, 9, seed=8))
    got = experiment_helper._ensemble_logits(stub, x, 2, None)
    assert stub.calls == [(2, 3, 6, 9), (1, 3, 6, 9)]
    assert torch.equal(got, experiment_helper._forward_logits(C.StubNet(), x, 2))


def test_passes_refuse_anything_but_ensemble_options(tmp_path):
    class Loader:
        dataset = []

        def __iter__(self):
            return iter([])

    for call in (experiment_helper.test_fast, experiment_helper.test_objects):
        provider = C.Provider(C.StubNet())
        with pytest.raises(ValueError) as err:
            call(provider if call is experiment_helper.test_fast else [provider], Loader(), tmp_path, ensemble={"flip": True})
        assert str(err.value) == "%s: ensemble must be a fosvos_hip.options.EnsembleOptions or None, got {'flip': True}" % call.__name__
