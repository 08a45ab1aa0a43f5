"""util/mask_crf.py, the numpy statement of the CRF on the frame: the vectorised form against the per-pixel loop bit for bit,
its degenerate cases, the guide levels, the tables and the belief at their ends, the ``Da == 0`` branch, CrfOptions and the
``--crf`` flags, ``test_fast(crf=)`` / ``test_objects(crf=)`` on CPU tensors against the definition, and the prototype case.
tests/mask_crf_cases.py holds the cases."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import guided_cases as G  # noqa: E402
import mask_crf_cases as C  # noqa: E402
from fosvos_hip import limits  # noqa: E402
from fosvos_hip.options import CleanOptions, CrfOptions, EnsembleOptions  # noqa: E402
from util import args_helper, experiment_helper, io_helper, mask_crf as M  # noqa: E402

NAN, INF = float("nan"), float("inf")


# ------------------------------------------------------------------------------------------ the two forms of the definition
@pytest.mark.parametrize("guide", C.GUIDES)
@pytest.mark.parametrize("shape, r, iterations", [((1, 1), 5, 2), ((3, 5), 5, 2), ((7, 9), 2, 3), ((2, 13), 1, 1), ((13, 14), 5, 2)])
def test_refine_is_the_loop_bit_for_bit(shape, r, iterations, guide):
    h, w = shape
    o = C.options(r, iterations, guide)
    im, x = C.image(1, h, w, guide)[0], C.logits(1, h, w)[0, 0]
    got, want = M.refine(im, x, o), M.refine_loop(im, x, o)
    assert got.dtype == np.float32 and got.shape == (h, w)
    assert C.same_bits(got, want) is None, C.same_bits(got, want)
    assert np.isfinite(got).all()
    assert np.abs(got).max() <= o.clip + o.weight_appearance + o.weight_smooth


def test_a_frame_is_its_own_guide():
    f = G.frames(1, 9, 11, "random")[0]
    x = C.logits(1, 9, 11)[0, 0]
    assert C.same_bits(M.refine(f, x), M.refine(C.prepared(f[None])[0], x)) is None
    assert C.same_bits(M.refine_loop(f, x, C.options(2, 1)), M.refine(C.prepared(f[None])[0], x, C.options(2, 1))) is None


def test_given_tables_are_the_ones_made():
    o = C.options(3, 2)
    im, x = C.image(1, 6, 7, "random")[0], C.logits(1, 6, 7)[0, 0]
    assert C.same_bits(M.refine(im, x, o, M.tables(o)), M.refine(im, x, o)) is None
    with pytest.raises(ValueError):
        M.refine(im, x, o, M.tables(C.options(2, 2)))        # another radius' vector
    with pytest.raises(ValueError):
        M.refine(im, x[:, :-1], o)


def clipped(x, clip):
    x = x.astype(np.float64)
    return np.where(np.isnan(x), -clip, np.clip(x, -clip, clip)).astype(np.float32)


def same_values(got, want):
    """Equal as numbers, bit for bit but for the sign of a zero: ``(u + w * 0.0) + w * 0.0`` of ``u = -0.0`` is ``+0.0``."""
    return got.dtype == want.dtype == np.float32 and np.array_equal(got, want) and \
        np.array_equal(C.bits(got)[want != 0], C.bits(want)[want != 0])


@pytest.mark.parametrize("guide", ("random", "nonfinite"))
def test_both_weights_zero_gives_the_clipped_logit(guide):
    o = C.options(4, 3, guide, weight_appearance=0.0, weight_smooth=0.0)
    im, x = C.image(1, 8, 9, guide)[0], C.logits(1, 8, 9)[0, 0]
    want = clipped(x, 6.0)
    assert np.isnan(x).any() and np.isinf(x).any()
    assert same_values(M.refine(im, x, o), want) and same_values(M.refine_loop(im, x, o), want)


@pytest.mark.parametrize("value", (0.0, -0.0, 2.5, -7.0, 1e30, INF, -INF, NAN))
def test_a_1x1_map_gives_the_clipped_logit(value):
    im = C.image(1, 1, 1, "random")[0]
    x = np.full((1, 1), value, dtype=np.float32)
    for refine in (M.refine, M.refine_loop):
        assert same_values(refine(im, x, C.options(5, 5)), clipped(x, 6.0))


# ------------------------------------------------------------------------------------------ guide levels
@pytest.mark.parametrize("shape", [(1, 1), (5, 7), (33, 67)])
def test_guide_levels_of_a_prepared_frame_are_its_bytes(shape):
    f = G.frames(2, shape[0], shape[1], "random")
    im = C.prepared(f)
    for k in range(2):
        assert np.array_equal(M.guide_levels(im[k]), f[k].transpose(2, 0, 1))
    every = np.arange(256, dtype=np.uint8).reshape(1, 16, 16, 1).repeat(3, axis=3)     # each byte in each channel
    assert np.array_equal(M.guide_levels(C.prepared(every)[0]), every[0].transpose(2, 0, 1))


def test_guide_levels_of_a_resampled_frame_are_bytes_too():
    from util import frame_resample as R
    f = G.frames(1, 12, 20, "random")[0]
    im = R.prepare_frame_scaled(f, 6, 10)[0]
    g = M.guide_levels(im)
    mean = np.array(M.MEANVAL, dtype=np.float32)
    assert g.dtype == np.uint8 and np.abs(g.astype(np.float64) - (im.astype(np.float64) + mean[:, None, None])).max() <= 0.5


def test_guide_levels_of_values_no_frame_has():
    x = np.zeros((3, 1, 6), dtype=np.float32)
    x[:, 0, :] = np.array([NAN, INF, -INF, 1e30, -1e30, 400.0], dtype=np.float32)
    assert np.array_equal(M.guide_levels(x)[:, 0], np.array([[0, 255, 0, 255, 0, 255]] * 3, dtype=np.uint8))
    with pytest.raises(ValueError):
        M.guide_levels(x.astype(np.float64))


# ------------------------------------------------------------------------------------------ tables and belief
def test_tables_at_their_ends():
    o = CrfOptions(radius=3, theta_pos=2.0, theta_rgb=13.0, theta_smooth=0.5)
    tab = M.tables(o)
    oa, ob, od, total = M.table_sizes(3)
    assert (oa, ob, od, total) == (256, 256 + 49, 256 + 98, 256 + 98 + 2049) and tab.shape == (total,) and tab.dtype == np.float64
    rgb, a, b, d = tab[:oa], tab[oa:ob].reshape(7, 7), tab[ob:od].reshape(7, 7), tab[od:]
    assert rgb[0] == 1.0 and rgb[255] == np.exp(-255.0 ** 2 / (2.0 * 13.0 ** 2)) and (np.diff(rgb) < 0).all()
    assert a[3, 3] == 1.0 and a[0, 0] == np.exp(-18.0 / 8.0) and a[3, 0] == np.exp(-9.0 / 8.0)
    assert np.array_equal(a, a.T) and np.array_equal(a, a[::-1, ::-1])
    assert b[3, 3] == 1.0 and b[6, 6] == np.exp(-18.0 / 0.5) and b[3, 4] == np.exp(-1.0 / 0.5)
    assert d[0] == np.tanh(-8.0) and d[2048] == np.tanh(8.0) and d[1024] == 0.0 and (np.diff(d) > 0).all()
    assert M.tables(CrfOptions(theta_rgb=1.0))[255] == 0.0      # the underflow the Da == 0 branch is for
    assert np.array_equal(M.tables(), M.tables(CrfOptions()))


def test_belief_at_and_beyond_its_ends():
    d = M.tables()[M.table_sizes(5)[2]:]
    z = np.array([-16.0, 16.0, -17.0, 1e300, -1e300, 0.0, -0.0, 1.0 / 128], dtype=np.float64)
    s = M.belief(z, d)
    assert s[0] == d[0] and s[1] == d[2048] and s[2] == d[0] and s[3] == d[2048] and s[4] == d[0]
    assert s[5] == 0.0 and s[6] == 0.0 and not np.signbit(s[5]) and not np.signbit(s[6])
    assert s[7] == d[1024] + 0.5 * (d[1025] - d[1024])
    zz = np.linspace(-20.0, 20.0, 4001)
    assert np.abs(M.belief(zz, d) - np.tanh(np.clip(zz, -16, 16) / 2.0)).max() < 2e-5


# ------------------------------------------------------------------------------------------ Da == 0
def test_an_isolated_pixel_has_no_appearance_mass():
    """Salt of 255 on 0 at ``theta_rgb`` 1: RGB[255] is 0, so every neighbour of a salt pixel weighs nothing.  The branch is
    reached - and there the appearance message is 0, so the pixel keeps the unary plus the smoothness message."""
    h, w = 13, 14
    o = C.options(5, 1, "salt")
    im, x = C.image(1, h, w, "salt")[0], C.logits(1, h, w)[0, 0]
    salt = C.salt_frames(1, h, w)[0, :, :, 0] == 255
    z, da = M.messages(im, x, o)
    assert salt.sum() == 4 and np.array_equal(da == 0.0, salt)
    without = M.messages(im, x, C.options(5, 1, "salt", weight_appearance=0.0))[0]
    assert np.array_equal(z[salt], without[salt]) and not np.array_equal(z[~salt], without[~salt])
    assert np.isfinite(z).all()
    assert C.same_bits(M.refine(im, x, o), M.refine_loop(im, x, o)) is None


# ------------------------------------------------------------------------------------------ options
def test_limits_equal_the_definitions():
    assert limits.CRF_MAX_ITERATIONS == M.MAX_ITERATIONS and limits.CRF_MAX_RADIUS == M.MAX_RADIUS
    assert limits.CRF_THETA_POS_RANGE == M.THETA_POS_RANGE and limits.CRF_THETA_RGB_RANGE == M.THETA_RGB_RANGE
    assert limits.CRF_THETA_SMOOTH_RANGE == M.THETA_SMOOTH_RANGE
    assert limits.CRF_MAX_WEIGHT == M.MAX_WEIGHT and limits.CRF_MAX_CLIP == M.MAX_CLIP
    assert M.Params()._asdict() == CrfOptions().as_dict()


def refused(call, message):
    with pytest.raises(ValueError) as e:
        call()
    assert str(e.value) == message


def test_crf_options():
    o = CrfOptions()
    assert o.as_dict() == {'iterations': 5, 'radius': 5, 'theta_pos': 8.0, 'theta_rgb': 13.0, 'theta_smooth': 3.0,
                           'weight_appearance': 4.0, 'weight_smooth': 3.0, 'clip': 6.0}
    assert CrfOptions(theta_pos=8) == o and hash(CrfOptions(theta_pos=8)) == hash(o)
    assert all(type(v) is float for k, v in CrfOptions(theta_pos=8, clip=6).as_dict().items() if k not in ('iterations', 'radius'))
    for field, good, bad, expect in (
            ("iterations", (1, 10), (0, 11, True, 5.0), "an integer in 1..10"),
            ("radius", (1, 5), (0, 6, True, 2.0), "an integer in 1..5"),
            ("theta_pos", (0.25, 1e3, 8), (float(np.nextafter(0.25, 0)), float(np.nextafter(1e3, INF)), True, NAN, INF),
             "a finite number in [0.25, 1000]"),
            ("theta_rgb", (1, 1.0, 1e3), (float(np.nextafter(1.0, 0)), 1000.5, False, NAN), "a finite number in [1, 1000]"),
            ("theta_smooth", (0.25, 1e3), (0.2, 1001, True, -INF), "a finite number in [0.25, 1000]"),
            ("weight_appearance", (0, 0.0, 100.0), (-5e-324, 100.5, True, NAN), "a finite number in [0, 100]"),
            ("weight_smooth", (0, 0.0, 100), (-1.0, 101, False, INF), "a finite number in [0, 100]"),
            ("clip", (5e-324, 1e4), (0.0, 0, float(np.nextafter(1e4, INF)), True, NAN), "a finite number in (0, 10000]")):
        for v in good:
            assert getattr(CrfOptions(**{field: v}), field) == v
            M.check_options(CrfOptions(**{field: v}))
        for v in bad:
            refused(lambda: CrfOptions(**{field: v}), f"CrfOptions: {field} must be {expect}, got {v!r}")
            with pytest.raises(ValueError):
                M.check_options(M.Params(**{field: v}))


# ------------------------------------------------------------------------------------------ the flags
def test_crf_flags_combine():
    a = args_helper.parse_args(True, ["--fast-test", "--crf"])
    assert a.crf_options == CrfOptions()
    a = args_helper.parse_args(True, ["--fast-test", "--crf", "--crf-iterations", "3", "--crf-radius", "2", "--crf-theta-pos", "4",
                                      "--crf-theta-rgb", "9.5", "--crf-theta-smooth", "1", "--crf-weight-appearance", "2",
                                      "--crf-weight-smooth", "0", "--crf-clip", "8"])
    assert a.crf_options == CrfOptions(iterations=3, radius=2, theta_pos=4.0, theta_rgb=9.5, theta_smooth=1.0,
                                       weight_appearance=2.0, weight_smooth=0.0, clip=8.0)
    a = args_helper.parse_args(True, ["--synthetic", "--multi-object", "--score", "--png-fitted", "--crf", "--ensemble-flip"])
    assert a.crf_options == CrfOptions() and a.ensemble == EnsembleOptions(flip=True)
    a = args_helper.parse_args(True, ["--fast-test", "--score", "--png-fitted", "--clean-largest", "--clean-min-area", "9",
                                      "--clean-temporal", "3", "--ensemble-scales", "0.75", "1", "--device-decode", "--crf",
                                      "--crf-radius", "3"])
    assert a.crf_options == CrfOptions(radius=3) and a.clean_largest and a.device_decode
    assert args_helper.parse_args(True, ["--fast-test"]).crf_options is None
    assert args_helper.parse_args(True, []).crf_options is None
    assert not hasattr(args_helper.parse_args(False, []), "crf_options")
    with pytest.raises(SystemExit):
        args_helper.parse_args(False, ["--crf"])      # an online flag


NEEDS_PASS = "--crf refines the logits of the device test pass: it needs --fast-test or --multi-object"


@pytest.mark.parametrize("argv, message", [
    (["--crf"], NEEDS_PASS),
    (["--crf", "--score"], NEEDS_PASS),
    (["--crf", "--adapt-steps", "1"], NEEDS_PASS),
    (["--fast-test", "--crf", "--adapt-steps", "2"],
     "--crf refines the answers of a frozen net; a CRF in the adaptive test pass (--adapt-steps) is not built"),
    (["--fast-test", "--crf", "--eval-speeds"],
     "--crf belongs to a PNG-writing test pass; --eval-speeds times one forward and writes nothing"),
    (["--fast-test", "--crf", "--data-parallel"],
     "--crf runs in the test pass on one device; --data-parallel spreads a training cycle over the ranks"),
    (["--fast-test", "--crf-iterations", "3"], "--crf-iterations set(s) an option of the CRF: it needs --crf"),
    (["--multi-object", "--crf-radius", "2", "--crf-clip", "5"], "--crf-radius / --crf-clip set(s) an option of the CRF: it needs --crf"),
    (["--crf-theta-pos", "2"], "--crf-theta-pos set(s) an option of the CRF: it needs --crf"),
    (["--crf-theta-rgb", "2"], "--crf-theta-rgb set(s) an option of the CRF: it needs --crf"),
    (["--crf-theta-smooth", "2"], "--crf-theta-smooth set(s) an option of the CRF: it needs --crf"),
    (["--crf-weight-appearance", "2"], "--crf-weight-appearance set(s) an option of the CRF: it needs --crf"),
    (["--crf-weight-smooth", "2"], "--crf-weight-smooth set(s) an option of the CRF: it needs --crf"),
    (["--fast-test", "--crf", "--crf-radius", "6"], "--crf-*: radius must be an integer in 1..5, got 6"),
    (["--fast-test", "--crf", "--crf-iterations", "0"], "--crf-*: iterations must be an integer in 1..10, got 0"),
    (["--fast-test", "--crf", "--crf-theta-rgb", "0.5"], "--crf-*: theta_rgb must be a finite number in [1, 1000], got 0.5"),
    (["--fast-test", "--crf", "--crf-clip", "0"], "--crf-*: clip must be a finite number in (0, 10000], got 0.0"),
    (["--fast-test", "--crf", "--crf-weight-smooth", "nan"], "--crf-*: weight_smooth must be a finite number in [0, 100], got nan"),
])
def test_crf_flag_refusals_say_why(argv, message, capsys):
    with pytest.raises(SystemExit):
        args_helper.parse_args(True, argv)
    assert capsys.readouterr().err.rstrip().split("error: ", 1)[1] == message


def test_online_main_passes_the_options(monkeypatch, tmp_path):
    import train_online
    seen = []

    def fake_pass(*args, **kwargs):
        seen.append(kwargs)
        raise KeyboardInterrupt

    monkeypatch.setattr(train_online.gpu_handler, "select_gpu", lambda *a, **k: None)
    monkeypatch.setattr(train_online, "crf", None)
    monkeypatch.setattr(train_online, "save_dir_models", tmp_path / "models")
    monkeypatch.setattr(train_online, "save_dir_results", tmp_path / "results")
    monkeypatch.setattr(train_online.io_helper, "write_settings", lambda *a, **k: None)
    monkeypatch.setattr(train_online, "_get_summary_writer", lambda *a, **k: None)
    monkeypatch.setattr(train_online.provider_mapping[("online", "vgg16")], "load_network_test", lambda self, sequence=None: None)
    monkeypatch.setattr(train_online.experiment_helper, "test_fast", fake_pass)
    common = ["--synthetic", "--height", "24", "--width", "40", "--no-training", "--fast-test"]
    with pytest.raises(KeyboardInterrupt):
        train_online.main(common + ["--crf", "--crf-radius", "2"])
    assert seen[-1]["crf"] == CrfOptions(radius=2) == train_online.crf
    with pytest.raises(KeyboardInterrupt):
        train_online.main(common)
    assert "crf" not in seen[-1] and train_online.crf is None      # absent: the call is what it was


# ------------------------------------------------------------------------------------------ the passes, host path
@pytest.mark.parametrize("extra", ["alone", "clean", "ensemble"])
def test_fast_with_a_crf_on_cpu_tensors(tmp_path, extra):
    """5 frames of 24x40 in groups of 3 and 2: the files and the score are those of the pass without ``crf`` over a net that
    applies the definition itself - to the merged logits behind an ensemble, in front of the cleaning."""
    import test_ensemble_cases as EC
    h, w = 24, 40
    crf = CrfOptions(iterations=2, radius=3)
    kw = {"clean": CleanOptions(largest=True)} if extra == "clean" else {}
    ens = EnsembleOptions(flip=True) if extra == "ensemble" else None

    def loader():
        return io_helper.get_data_loader_test(None, 1, "blob", synthetic=(h, w), n_frames=5)

    stub = C.StubNet()
    data = loader()
    score = experiment_helper.test_fast(C.Provider(stub), data, tmp_path / "crf", data.dataset.annotation, group=3, seq_name="blob",
                                        crf=crf, **kw, **({"ensemble": ens} if ens else {}))
    assert score["crf"] == crf.as_dict() == experiment_helper.last_fast["crf"]
    assert experiment_helper.last_fast["group_sizes"] == [3, 2]
    inner = C.StubNet() if ens is None else EC.EnsembleByDefinition(C.StubNet(), ens.views())
    data = loader()
    want = experiment_helper.test_fast(C.Provider(C.CrfByDefinition(inner, crf)), data, tmp_path / "definition",
                                       data.dataset.annotation, group=3, seq_name="blob", **kw)
    assert "crf" not in want and "crf" not in experiment_helper.last_fast
    files = C.files_of(tmp_path / "crf")
    assert sorted(files) == ["blob/%05d.png" % k for k in range(5)] and files == C.files_of(tmp_path / "definition")
    for key in ("counts", "J", "F", "J_stats", "F_stats", "J&F", "fnames", "scored"):
        assert score[key] == want[key], key
    # ... and they are not the files of the pass without it, whose call is what it was
    data = loader()
    plain = experiment_helper.test_fast(C.Provider(C.StubNet()), data, tmp_path / "plain", data.dataset.annotation, group=3,
                                        seq_name="blob", crf=None, **kw)
    assert C.files_of(tmp_path / "plain") != files and "crf" not in plain


def test_fast_call_order_on_cpu_tensors(tmp_path, monkeypatch):
    """Per group: the ensemble's merge, ONE refinement of the whole group on the uploaded frames, then the cleaning."""
    from util import mask_components, test_ensemble
    log = []

    def logged(module, name):
        original = getattr(module, name)
        monkeypatch.setattr(module, name, lambda *a, **kw: (log.append(name), original(*a, **kw))[1])

    logged(test_ensemble, "merge")
    logged(M, "refine_batch")
    logged(mask_components, "clean_sequence")
    data = io_helper.get_data_loader_test(None, 1, "blob", synthetic=(12, 20), n_frames=3)
    experiment_helper.test_fast(C.Provider(C.StubNet()), data, tmp_path, None, group=2, seq_name="blob",
                                crf=CrfOptions(iterations=1, radius=1), ensemble=EnsembleOptions(flip=True),
                                clean=CleanOptions(largest=True))
    assert log == ["merge", "refine_batch", "clean_sequence"] * 2


def test_objects_with_a_crf_on_cpu_tensors(tmp_path, monkeypatch):
    """3 nets, 4 frames in groups of 3 and 1: every net's logits are refined, once a group, before the labels are merged."""
    from dataloaders.synthetic import SyntheticObjectsSequence
    from torch.utils.data import DataLoader
    from util import object_merge
    h, w = 24, 40
    crf = CrfOptions(iterations=2, radius=2)
    data = SyntheticObjectsSequence("blobs", h, w, n_frames=4, n_objects=3)

    def loader():
        return DataLoader(data, batch_size=1, shuffle=False, num_workers=0)

    def stubs():
        return [C.StubNet(channel=k, scale=0.125 + 0.05 * k) for k in range(3)]

    log = []
    for module, name in ((experiment_helper, "_crf_logits"), (object_merge, "merge_labels")):
        original = getattr(module, name)
        monkeypatch.setattr(module, name, lambda *a, _o=original, _n=name, **kw: (log.append(_n), _o(*a, **kw))[1])
    score = experiment_helper.test_objects([C.Provider(s) for s in stubs()], loader(), tmp_path / "crf", data.annotation, group=3,
                                           seq_name="blobs", crf=crf)
    assert log == (["_crf_logits"] * 3 + ["merge_labels"]) * 2
    assert score["crf"] == crf.as_dict() and score["n_objects"] == 3
    want = experiment_helper.test_objects([C.Provider(C.CrfByDefinition(s, crf)) for s in stubs()], loader(), tmp_path / "definition",
                                          data.annotation, group=3, seq_name="blobs")
    assert "crf" not in want
    files = C.files_of(tmp_path / "crf")
    assert sorted(files) == ["blobs/%05d.png" % k for k in range(4)] and files == C.files_of(tmp_path / "definition")
    assert [o["counts"] for o in score["objects"]] == [o["counts"] for o in want["objects"]]
    assert score["J&F"] == want["J&F"]
    experiment_helper.test_objects([C.Provider(s) for s in stubs()], loader(), tmp_path / "plain", data.annotation, group=3,
                                   seq_name="blobs")
    assert C.files_of(tmp_path / "plain") != files


def test_passes_refuse_anything_but_crf_options(tmp_path):
    class Loader:
        dataset = []

        def __iter__(self):
            return iter([])

    for call in (experiment_helper.test_fast, experiment_helper.test_objects):
        provider = C.Provider(C.StubNet())
        with pytest.raises(ValueError) as err:
            call(provider if call is experiment_helper.test_fast else [provider], Loader(), tmp_path, crf={"radius": 2})
        assert str(err.value) == "%s: crf must be a fosvos_hip.options.CrfOptions or None, got {'radius': 2}" % call.__name__


# ------------------------------------------------------------------------------------------ the prototype case
def test_the_prototype_case_snaps_to_the_ellipse_and_loses_the_blob():
    """97 x 161, the net's mask three pixels off, a stray 4 x 5 blob: with the defaults the IoU with the truth rises (0.9222 ->
    0.9871 here) and the blob goes.  The asserted property is the strict rise; the figures are DESIGN.md's."""
    frame, truth, lg = C.prototype_case()
    before = C.iou(lg >= 0, truth)
    out = M.refine(frame, lg)
    after = C.iou(out >= 0, truth)
    print("prototype case: IoU %.4f -> %.4f" % (before, after))
    assert (lg[C.BLOB] >= 0).all() and not (out[C.BLOB] >= 0).any()
    assert after > before
    assert C.same_bits(out, M.refine(C.prepared(frame[None])[0], lg)) is None


def test_signed_distance_needs_only_numpy():
    m = np.zeros((7, 9), dtype=bool)
    m[2:5, 3:7] = True
    d = C.signed_distance(m)
    assert d[3, 4] == 2.0 and d[2, 3] == 1.0 and d[0, 0] == -np.sqrt(13.0) and d[3, 8] == -2.0 and d[6, 4] == -2.0
    assert ((d > 0) == m).all()
