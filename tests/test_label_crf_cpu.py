"""util/label_crf.py, the numpy statement of the joint CRF over the objects of a frame: the vectorised form against the
per-pixel loop bit for bit, its two degenerate cases (both weights 0: ``merge_labels``; one object: the binary CRF within its
tables' error), the tie rule through the whole arithmetic, the beliefs, the ``Da == 0`` branch, the two-object prototype case,
the refusals, ``test_objects(crf_joint=True)`` on CPU tensors against the definition and the ``--crf-joint`` flag.
tests/label_crf_cases.py holds the cases."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import guided_cases as G  # noqa: E402
import label_crf_cases as L  # noqa: E402
import mask_crf_cases as C  # noqa: E402
from fosvos_hip import limits  # noqa: E402
from fosvos_hip.options import CrfOptions, EnsembleOptions  # noqa: E402
from util import args_helper, experiment_helper, label_crf as LC, mask_crf as M, object_merge  # noqa: E402

NAN, INF = float("nan"), float("inf")


# ------------------------------------------------------------------------------------------ the two forms of the definition
@pytest.mark.parametrize("guide", L.GUIDES)
@pytest.mark.parametrize("shape, r, iterations, k", [((1, 1), 5, 2, 1), ((3, 5), 5, 2, 2), ((7, 9), 2, 3, 3), ((2, 13), 1, 1, 16),
                                                     ((9, 8), 5, 2, 5)])
def test_refine_labels_is_the_loop_bit_for_bit(shape, r, iterations, k, guide):
    h, w = shape
    o = C.options(r, iterations, guide)
    im, maps = C.image(1, h, w, guide)[0], [x[0, 0] for x in L.logit_maps(1, h, w, k)]
    labels, scores = LC.refine_labels(im, maps, o)
    want_labels, want_scores = LC.refine_labels_loop(im, maps, o)
    assert labels.dtype == np.uint8 and labels.shape == (h, w) and scores.dtype == np.float32 and scores.shape == (k + 1, h, w)
    assert np.array_equal(labels, want_labels)
    assert C.same_bits(scores, want_scores) is None, C.same_bits(scores, want_scores)
    assert np.isfinite(scores).all() and labels.max() <= k
    assert np.abs(scores).max() <= o.clip + o.weight_appearance + o.weight_smooth


def test_batch_is_frame_by_frame_and_a_frame_is_its_own_guide():
    n, h, w, k = 2, 6, 9, 3
    o = C.options(2, 2)
    f = G.frames(n, h, w, "random")
    im, maps = C.prepared(f), L.logit_maps(n, h, w, k)
    labels, scores = LC.refine_labels_batch(im, maps, o)
    assert labels.shape == (n, h, w) and labels.dtype == np.uint8 and scores.shape == (n, k + 1, h, w)
    for i in range(n):
        one = LC.refine_labels(f[i], [x[i, 0] for x in maps], o, LC.tables(o))
        assert np.array_equal(labels[i], one[0]) and C.same_bits(scores[i], one[1]) is None
    z, _ = LC.messages(im[0], [x[0, 0] for x in maps], o)
    assert z.dtype == np.float64 and C.same_bits(z.astype(np.float32), scores[0]) is None
    assert np.array_equal(LC.choose(z), labels[0])


def test_tables_share_everything_but_the_last_block():
    for r in (1, 5):
        o = C.options(r, 1, theta_rgb=7.0)
        mine, theirs = LC.tables(o), M.tables(o)
        od = M.table_sizes(r)[2]
        assert mine.dtype == np.float64 and mine.shape == theirs.shape
        assert np.array_equal(mine[:od], theirs[:od])
        e = mine[od:]
        assert e.size == 2049 and e[0] == 1.0 and e[64] == np.exp(-1.0) and e[2048] == np.exp(-32.0)
        assert (np.diff(e) < 0).all()


# ------------------------------------------------------------------------------------------ the beliefs
def test_beliefs_sum_to_one_and_the_sum_of_e_is_at_least_one():
    """``S`` is a running float64 sum of L terms: L - 1 roundings of at most 2^-53 of it each, and every ``q_l = e_l / S`` adds
    half an ulp of its own, 2^-53 over all of them.  So the exact sum of the beliefs is within ``L 2^-53`` of 1: within 1e-15
    for up to 8 labels (8.9e-16), which is asserted there, and within 1.9e-15 at the 17 labels of 16 objects (1.1e-15 was seen)."""
    ee = M._split_tables(LC.tables(), M.check_options())[3]
    rng = np.random.default_rng(5)
    z = rng.uniform(-13.0, 13.0, (17, 40, 50))
    z[:, 0, :5] = 0.0                 # every label equal
    z[0, 1, :] = 13.0
    z[1:, 1, :] = -13.0               # one label far above the rest
    z[3, 2, :] = z[5, 2, :]           # two labels equal
    z[:, 3, 0] = [-0.0, 0.0] * 8 + [-0.0]
    for n_labels in (2, 3, 8, 17):
        q, s = LC.beliefs(z[:n_labels], ee)
        assert q.shape == (n_labels, 40, 50) and (s >= 1.0).all() and (s <= n_labels).all()
        # (summed exactly: a float64 running sum of the beliefs would add roundings of its own)
        totals = np.array([math.fsum(column) for column in q.reshape(n_labels, -1).T.tolist()])
        assert np.abs(totals - 1.0).max() <= (1e-15 if n_labels <= 8 else n_labels * 2.0 ** -53)
        assert (q >= 0.0).all() and (q <= 1.0).all()
        assert np.array_equal(q[:, 0, :5], np.full((n_labels, 5), 1.0 / n_labels))
        assert np.array_equal(q[:, 3, 0], np.full(n_labels, 1.0 / n_labels))
    q, _ = LC.beliefs(z, ee)
    assert np.array_equal(q[3, 2], q[5, 2])
    # a gap beyond the table's end is the table's end: exp(-32)
    q, s = LC.beliefs(np.array([[0.0], [-200.0]]), ee)
    assert s[0] == 1.0 + np.exp(-32.0) and q[1, 0] == np.exp(-32.0) / s[0]
    # against the soft-max itself, to the tables' error
    q, _ = LC.beliefs(z[:5], ee)
    exact = np.exp(z[:5] - z[:5].max(axis=0))
    assert np.abs(q - exact / exact.sum(axis=0)).max() < 4e-5


# ------------------------------------------------------------------------------------------ the two degenerate cases
@pytest.mark.parametrize("k", [1, 2, 5])
def test_both_weights_zero_is_merge_labels(k):
    """Logits within the clip and NaN (never valid in either): the labels are ``merge_labels``' exactly.  Signed zeros are
    valid in both.  Beyond the clip the two differ by design (the clip makes ties), which the last lines pin."""
    n, h, w = 2, 9, 14
    o = CrfOptions(iterations=3, radius=2, weight_appearance=0.0, weight_smooth=0.0, clip=6.0)
    maps = L.logit_maps(n, h, w, k)
    maps = [np.where(np.isnan(x), x, np.clip(x, -6.0, 6.0)).astype(np.float32) for x in maps]
    assert any(np.isnan(x).any() for x in maps) and any((x == 0).any() for x in maps) and any((x == 6.0).any() for x in maps)
    im = C.image(n, h, w, "random")
    labels, scores = LC.refine_labels_batch(im, maps, o)
    assert np.array_equal(labels, object_merge.merge_labels([x[:, 0] for x in maps]))
    assert (scores[:, 0] == 0.0).all()
    for j, x in enumerate(maps):
        assert np.array_equal(scores[:, j + 1], np.where(np.isnan(x[:, 0]), np.float32(-6.0), x[:, 0]))
    # +-inf are the clip: +inf is an object, -inf is not; two nets beyond the clip tie and the lower one wins
    im1 = C.image(1, 1, 4, "random")
    a = np.array([[[[INF, -INF, 7.0, -0.0]]]], dtype=np.float32)
    b = np.array([[[[INF, -INF, 8.0, 0.0]]]], dtype=np.float32)
    assert LC.refine_labels_batch(im1, [a, b], o)[0].tolist() == [[[1, 0, 1, 1]]]
    assert object_merge.merge_labels([a[:, 0], b[:, 0]]).tolist() == [[[1, 0, 2, 1]]]


def test_one_object_is_the_binary_crf_within_the_tables_error():
    """K = 1 on the binary CRF's prototype case with the defaults: ``z_1 - z_0`` is the binary ``z`` to 1.4e-5 (the two
    piecewise-linear tables), and the labels are ``refine >= 0`` wherever the binary ``|z|`` is at least 1e-3."""
    frame, _, x = C.prototype_case()
    zb, _ = M.messages(frame, x)
    z, _ = LC.messages(frame, [x])
    gap = np.abs((z[1] - z[0]) - zb).max()
    print("largest |(z_1 - z_0) - z_binary| = %.3e" % gap)
    assert gap < 1e-4
    labels, _ = LC.refine_labels(frame, [x])
    sure = np.abs(zb) >= 1e-3
    assert sure.mean() >= 0.99
    assert np.array_equal(labels[sure] == 1, M.refine(frame, x)[sure] >= 0)


def test_equal_nets_stay_equal_and_the_lower_one_wins():
    """Nets j < k with identical logit maps over a constant guide: ``z_j`` and ``z_k`` are bit-identical after every iteration,
    and wherever they lead the label is j."""
    h, w = 11, 13
    im = C.image(1, h, w, "constant")[0]
    maps = [x[0, 0] for x in L.logit_maps(1, h, w, 2)]
    same = np.ascontiguousarray(maps[0] + np.float32(0.5))
    for order, (j, k) in (([maps[1], same, maps[0], same], (2, 4)), ([same, same], (1, 2)), ([same, maps[1], same], (1, 3))):
        for iterations in (1, 3):
            labels, scores = LC.refine_labels(im, order, C.options(3, iterations))
            assert C.same_bits(scores[j], scores[k]) is None
            assert not (labels == k).any() and (labels == j).any()
            if len(order) == 2:
                z, _ = LC.messages(im, order, C.options(3, iterations))
                assert np.array_equal(z[1], z[2]) and np.array_equal(labels == 1, z[1] >= z[0])


def test_the_salt_guide_reaches_the_empty_appearance_kernel():
    n, h, w, r, k = L.GPU_CASES[3]
    im, maps, o, tab, _, scores = L.reference(L.GPU_CASES[3], "salt", 1)
    z, da = LC.messages(im[0], [x[0, 0] for x in maps], o, tab)
    assert np.array_equal(da == 0.0, C.salt_frames(n, h, w)[0, :, :, 0] == 255) and (da == 0.0).sum() >= 6
    assert np.isfinite(z).all()


# ------------------------------------------------------------------------------------------ the prototype case
def test_two_instances_that_look_alike_are_told_apart():
    """97 x 161, two touching ellipses of nearly the same colour; each net answers on both, 1.5 lower on the other one, logit
    noise of sigma 1.5; default options.  IoU of object 1 / object 2 (README.md):
    ``merge_labels`` alone 0.568 / 0.544; per-net ``mask_crf.refine`` + ``merge_labels`` 0.612 / 0.591; the joint CRF 0.998 /
    0.998."""
    frame, truth, logits = L.two_object_case()
    merged = L.object_ious(object_merge.merge_labels([x[None] for x in logits])[0], truth)
    per_net = L.object_ious(object_merge.merge_labels([M.refine(frame, x)[None] for x in logits])[0], truth)
    joint = L.object_ious(LC.refine_labels(frame, logits)[0], truth)
    print("merge %.3f / %.3f, per net + merge %.3f / %.3f, joint %.3f / %.3f" % (*merged, *per_net, *joint))
    assert min(joint) >= 0.95
    assert max(per_net) <= 0.80
    assert max(merged) <= max(per_net)


# ------------------------------------------------------------------------------------------ refusals
def test_the_definition_refuses_what_it_cannot_take():
    im = C.image(1, 4, 5, "random")[0]
    x = C.logits(1, 4, 5)[0, 0]
    for bad, message in (([], "0 logit maps, outside [1, 16]"), ([x] * 17, "17 logit maps, outside [1, 16]")):
        with pytest.raises(ValueError) as err:
            LC.refine_labels(im, bad)
        assert str(err.value) == message
    with pytest.raises(ValueError) as err:
        LC.refine_labels(im, [x, x[:, :-1]])
    assert str(err.value) == "the guide is (4, 5), a logit map is (4, 4)"
    with pytest.raises(ValueError):
        LC.refine_labels(im, [x.astype(np.float64)])
    with pytest.raises(ValueError):
        LC.refine_labels(im, [x], C.options(3, 1), LC.tables(C.options(2, 1)))     # another radius' vector
    with pytest.raises(ValueError) as err:
        LC.refine_labels(im, [x], M.Params(radius=6))
    assert str(err.value) == "radius must be an integer in 1..5, got 6"
    with pytest.raises(ValueError):
        LC.refine_labels_batch(im[None], [x[None]])                                 # [N,H,W] is no [N,1,H,W]
    with pytest.raises(ValueError):
        LC.refine_labels_batch(im[None], [np.stack([x, x])[:, None]])               # two frames of logits for one image
    assert LC.MAX_OBJECTS == object_merge.MAX_OBJECTS == limits.MAX_OBJECTS


# ------------------------------------------------------------------------------------------ the pass, host path
H, W = 24, 40


def object_data(n_frames=4, n_objects=3):
    from dataloaders.synthetic import SyntheticObjectsSequence
    return SyntheticObjectsSequence("blobs", H, W, n_frames=n_frames, n_objects=n_objects)


def loader(data):
    from torch.utils.data import DataLoader
    return DataLoader(data, batch_size=1, shuffle=False, num_workers=0)


def stubs(k=3):
    return [C.StubNet(channel=j % 3, scale=0.125 + 0.05 * j) for j in range(k)]


@pytest.mark.parametrize("extra", ["alone", "ensemble"])
def test_objects_with_a_joint_crf_on_cpu_tensors(tmp_path, extra):
    """3 nets, 4 frames in groups of 3 and 1: the files and the counts are those of the pass without a CRF over nets that
    answer with the definition's label maps - of the merged logits behind an ensemble."""
    import test_ensemble_cases as EC
    crf = CrfOptions(iterations=2, radius=2)
    ens = EnsembleOptions(flip=True) if extra == "ensemble" else None
    data = object_data()
    score = experiment_helper.test_objects([C.Provider(s) for s in stubs()], loader(data), tmp_path / "joint", data.annotation,
                                           group=3, seq_name="blobs", crf=crf, crf_joint=True,
                                           **({"ensemble": ens} if ens else {}))
    assert score["crf"] == crf.as_dict() and score["crf_joint"] is True and score["n_objects"] == 3
    assert experiment_helper.last_score["crf_joint"] is True
    inner = stubs() if ens is None else [EC.EnsembleByDefinition(s, ens.views()) for s in stubs()]
    nets = [C.Provider(L.JointByDefinition(inner, j, crf)) for j in range(3)]
    want = experiment_helper.test_objects(nets, loader(data), tmp_path / "definition", data.annotation, group=3, seq_name="blobs")
    assert "crf" not in want and "crf_joint" not in want
    files = C.files_of(tmp_path / "joint")
    assert sorted(files) == ["blobs/%05d.png" % k for k in range(4)] and files == C.files_of(tmp_path / "definition")
    assert [o["counts"] for o in score["objects"]] == [o["counts"] for o in want["objects"]]
    assert score["J&F"] == want["J&F"]
    if ens is None:
        # ... and they are neither the files of the per-net CRF nor those of the pass without one
        for name, kw in (("per_net", {"crf": crf}), ("plain", {})):
            other = experiment_helper.test_objects([C.Provider(s) for s in stubs()], loader(data), tmp_path / name, data.annotation,
                                                   group=3, seq_name="blobs", **kw)
            assert C.files_of(tmp_path / name) != files and "crf_joint" not in other


def test_objects_call_order_on_cpu_tensors(tmp_path, monkeypatch):
    """Per group ONE ``refine_labels_batch`` in the place of the K refinements and of the merge; without the argument the
    sequence is what it was."""
    data = object_data(n_frames=3)
    crf = CrfOptions(iterations=1, radius=1)
    log = []
    for module, name in ((experiment_helper, "_crf_logits"), (object_merge, "merge_labels"), (LC, "refine_labels_batch"),
                         (M, "refine_batch")):
        original = getattr(module, name)
        monkeypatch.setattr(module, name, lambda *a, _o=original, _n=name, **kw: (log.append(_n), _o(*a, **kw))[1])
    run = lambda **kw: experiment_helper.test_objects([C.Provider(s) for s in stubs()], loader(data), tmp_path, data.annotation,  # noqa: E731
                                                      group=2, seq_name="blobs", **kw)
    run(crf=crf, crf_joint=True)
    assert log == ["refine_labels_batch"] * 2
    del log[:]
    score = run(crf=crf)
    assert log == (["_crf_logits", "refine_batch"] * 3 + ["merge_labels"]) * 2 and "crf_joint" not in score
    del log[:]
    score = run(crf=crf, crf_joint=False)
    assert log == (["_crf_logits", "refine_batch"] * 3 + ["merge_labels"]) * 2 and "crf_joint" not in score
    del log[:]
    score = run()
    assert log == ["merge_labels"] * 2 and "crf" not in score and "crf_joint" not in score


def test_objects_refuses_a_joint_crf_without_options(tmp_path):
    class Loader:
        dataset = []

        def __iter__(self):
            return iter([])

    with pytest.raises(ValueError) as err:
        experiment_helper.test_objects([C.Provider(C.StubNet())], Loader(), tmp_path, crf_joint=True)
    assert str(err.value) == "test_objects: crf_joint is the joint form of the CRF: it needs crf (a CrfOptions)"
    with pytest.raises(ValueError) as err:
        experiment_helper.test_objects([C.Provider(C.StubNet())], Loader(), tmp_path, crf=CrfOptions(), crf_joint=1)
    assert str(err.value) == "test_objects: crf_joint must be a bool, got 1"


# ------------------------------------------------------------------------------------------ the flag
def test_the_flag_combines_with_what_crf_combines_with():
    a = args_helper.parse_args(True, ["--multi-object", "--crf", "--crf-joint"])
    assert a.crf_joint is True and a.crf_options == CrfOptions()
    a = args_helper.parse_args(True, ["--synthetic", "--multi-object", "--score", "--png-fitted", "--crf", "--crf-joint", "--ensemble-flip",
                                      "--crf-radius", "3", "--objects", "3"])
    assert a.crf_joint is True and a.crf_options == CrfOptions(radius=3) and a.ensemble == EnsembleOptions(flip=True)
    assert args_helper.parse_args(True, ["--multi-object", "--crf"]).crf_joint is False
    assert args_helper.parse_args(True, []).crf_joint is False
    assert not hasattr(args_helper.parse_args(False, []), "crf_joint")
    with pytest.raises(SystemExit):
        args_helper.parse_args(False, ["--crf-joint"])      # an online flag


NEEDS_CRF = "--crf-joint is the joint form of the CRF: it needs --crf"
NEEDS_OBJECTS = ("--crf-joint lets the objects of a frame compete: it needs --multi-object (the single-object pass of --fast-test has "
                 "one object)")


@pytest.mark.parametrize("argv, message", [
    (["--crf-joint"], NEEDS_CRF),
    (["--multi-object", "--crf-joint"], NEEDS_CRF),
    (["--fast-test", "--crf-joint"], NEEDS_CRF),
    (["--fast-test", "--crf", "--crf-joint"], NEEDS_OBJECTS),
    (["--crf", "--crf-joint"], NEEDS_OBJECTS),
    (["--multi-object", "--crf", "--crf-joint", "--crf-iterations", "11"], "--crf-*: iterations must be an integer in 1..10, got 11"),
    (["--multi-object", "--crf", "--crf-joint", "--crf-clip", "0"], "--crf-*: clip must be a finite number in (0, 10000], got 0.0"),
])
def test_flag_refusals_say_why(argv, message, capsys):
    with pytest.raises(SystemExit):
        args_helper.parse_args(True, argv)
    assert capsys.readouterr().err.rstrip().split("error: ", 1)[1] == message


@pytest.mark.parametrize("extra", [["--adapt-steps", "2"], ["--eval-speeds"], ["--data-parallel"]])
def test_the_flag_goes_nowhere_crf_does_not(extra, capsys):
    """What ``--crf`` is refused with under ``--multi-object`` stays refused with the flag, and with the same reason (the
    multi-object pass refuses these before the CRF is looked at)."""
    reasons = []
    for flags in (["--crf"], ["--crf", "--crf-joint"]):
        with pytest.raises(SystemExit):
            args_helper.parse_args(True, ["--multi-object"] + flags + extra)
        reasons.append(capsys.readouterr().err.rstrip().split("error: ", 1)[1])
    assert reasons[0] == reasons[1]


def test_online_main_passes_the_flag(monkeypatch, tmp_path):
    import train_online
    seen = []

    def fake_pass(*args, **kwargs):
        seen.append(kwargs)
        raise KeyboardInterrupt

    monkeypatch.setattr(train_online.gpu_handler, "select_gpu", lambda *a, **k: None)
    monkeypatch.setattr(train_online, "crf", None)
    monkeypatch.setattr(train_online, "crf_joint", False)
    monkeypatch.setattr(train_online, "save_dir_models", tmp_path / "models")
    monkeypatch.setattr(train_online, "save_dir_results", tmp_path / "results")
    monkeypatch.setattr(train_online.io_helper, "write_settings", lambda *a, **k: None)
    monkeypatch.setattr(train_online, "_get_summary_writer", lambda *a, **k: None)
    monkeypatch.setattr(train_online.provider_mapping[("online", "vgg16")], "load_network_test", lambda self, sequence=None: None)
    monkeypatch.setattr(train_online.experiment_helper, "test_objects", fake_pass)
    common = ["--synthetic", "--height", "24", "--width", "40", "--no-training", "--multi-object"]
    with pytest.raises(KeyboardInterrupt):
        train_online.main(common + ["--crf", "--crf-joint", "--crf-radius", "2"])
    assert seen[-1]["crf"] == CrfOptions(radius=2) and seen[-1]["crf_joint"] is True and train_online.crf_joint is True
    with pytest.raises(KeyboardInterrupt):
        train_online.main(common + ["--crf"])
    assert "crf_joint" not in seen[-1] and train_online.crf_joint is False      # absent: the call is what it was
    with pytest.raises(KeyboardInterrupt):
        train_online.main(common)
    assert "crf" not in seen[-1] and "crf_joint" not in seen[-1]
