"""The DAVIS 2016 measures on the host (util/davis_measures.py), the scored test pass on CPU tensors
(util/experiment_helper.test_scored with its numpy path) and the --score flag.  The counts of the small cases are worked
out by hand in the comments; the pinned ellipse pair can be recomputed by anyone from its two formulas."""
import os
import sys

import numpy as np
import pytest
import torch
import yaml
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from util import args_helper, davis_measures as M, experiment_helper, io_helper  # noqa: E402
from test_resident_set_cpu import SEQS, write_davis_tree  # noqa: E402


def rect(h, w, y0, y1, x0, x1):
    m = np.zeros((h, w), dtype=bool)
    m[y0:y1, x0:x1] = True
    return m


# ------------------------------------------------------------------------------------------ counts and J / F
def test_boundary_map_of_a_rectangle():
    # rows 2..4, columns 3..6 of a 8x10 grid.  A pixel is set when its right, lower or lower-right neighbour differs:
    # row 1 (above the box): columns 2..6 (the lower / lower-right neighbour is inside)            -> 5
    # rows 2, 3: column 2 (right neighbour inside) and column 6 (right neighbour outside)          -> 2 each
    # row 4 (the box's last): columns 2..6 (2: right differs; 3..6: lower neighbour outside)       -> 5
    b = M.boundary_map(rect(8, 10, 2, 5, 3, 7))
    want = np.zeros((8, 10), dtype=bool)
    want[1, 2:7] = True
    want[2, [2, 6]] = True
    want[3, [2, 6]] = True
    want[4, 2:7] = True
    assert np.array_equal(b, want) and b.sum() == 14


def test_boundary_map_last_row_last_column_corner():
    s = np.zeros((3, 4), dtype=bool)
    s[2, 3] = True  # the corner pixel alone
    b = M.boundary_map(s)
    # (1,2): lower-right differs; (1,3) last column: lower differs; (2,2) last row: right differs; the corner itself: never
    want = np.zeros((3, 4), dtype=bool)
    want[1, 2] = want[1, 3] = want[2, 2] = True
    assert np.array_equal(b, want)


def test_identical_masks():
    a = rect(12, 15, 3, 8, 4, 11)
    c = M.jf_counts_numpy(a, a, 1)
    assert c[0] == c[1] == 35 and c[2] == c[3] == c[4] == c[5]
    j, f = M.jf_from_counts(c)
    assert j == 1.0 and f == 1.0


def test_disjoint_masks():
    a, b = rect(20, 30, 2, 6, 2, 6), rect(20, 30, 12, 17, 20, 26)
    c = M.jf_counts_numpy(a, b, 2)
    assert list(c[:2]) == [0, 16 + 30] and c[4] == 0 and c[5] == 0 and c[2] > 0 and c[3] > 0
    j, f = M.jf_from_counts(c)
    assert j == 0.0 and f == 0.0


def test_both_empty_and_one_empty():
    z, a = np.zeros((9, 9), dtype=bool), rect(9, 9, 2, 5, 2, 5)
    c = M.jf_counts_numpy(z, z, 1)
    assert list(c) == [0] * 6
    assert M.jf_from_counts(c) == (1.0, 1.0)
    # prediction empty, ground truth not: J = 0, P = 1, R = 0 -> F = 0
    c = M.jf_counts_numpy(z, a, 1)
    assert list(c[:3]) == [0, 9, 0] and c[3] > 0 and c[4] == 0 and c[5] == 0
    assert M.jf_from_counts(c) == (0.0, 0.0)
    # ground truth empty, prediction not: J = 0, P = 0, R = 1 -> F = 0
    c = M.jf_counts_numpy(a, z, 1)
    assert list(c[:2]) == [0, 9] and c[2] > 0 and c[3] == 0
    assert M.jf_from_counts(c) == (0.0, 0.0)


def test_precision_recall_conventions():
    # counts: inter, union, n_pred_b, n_gt_b, match_pred, match_gt
    j, f = M.jf_from_counts(np.array([[4, 8, 10, 20, 5, 20],    # P = 0.5, R = 1 -> F = 2/3
                                      [0, 0, 0, 0, 0, 0],       # both boundary maps empty -> F = 1
                                      [5, 5, 0, 3, 0, 0],       # only the predicted one empty: P = 1, R = 0 -> F = 0
                                      [5, 5, 3, 0, 0, 0],       # only the ground truth's empty: P = 0, R = 1 -> F = 0
                                      [1, 2, 4, 4, 0, 0]]))     # P = R = 0 -> F = 0
    assert np.allclose(j, [0.5, 1, 1, 1, 0.5]) and np.allclose(f, [2 / 3, 1, 0, 0, 0])


def test_full_frame_mask_has_no_boundary():
    full = np.ones((7, 11), dtype=bool)
    assert M.boundary_map(full).sum() == 0
    c = M.jf_counts_numpy(full, full, 3)
    assert list(c) == [77, 77, 0, 0, 0, 0]
    assert M.jf_from_counts(c) == (1.0, 1.0)


def test_rectangle_shifted_by_one_pixel_radius_one():
    # A = rows 2..4, columns 3..6 of an 8x12 grid (the rectangle of the first test), B = A moved one column right (4..7).
    # inter = 3 rows x columns 4..6 = 9, union = 3 x columns 3..7 = 15.
    # bmap(A): row 1: 2..6, rows 2,3: {2,6}, row 4: 2..6 (14 pixels); bmap(B): the same one column right (3..7, {3,7}).
    # r = 1: the disk is the pixel and its four edge neighbours.
    # match_pred = pixels of bmap(A) within the disk of a pixel of bmap(B):
    #   row 1: A's 2..6 against B's 3..7 in the same row: 2 is next to 3 -> all five match                     -> 5
    #   rows 2,3: A's 2 is next to B's 3; A's 6 is next to B's 7                                               -> 2 each
    #   row 4: as row 1                                                                                        -> 5
    # all 14 match, and by symmetry all 14 of bmap(B) match too.
    a, b = rect(8, 12, 2, 5, 3, 7), rect(8, 12, 2, 5, 4, 8)
    assert list(M.jf_counts_numpy(a, b, 1)) == [9, 15, 14, 14, 14, 14]
    # moved two columns (5..8) instead: bmap(B) = row 1: 4..8, rows 2,3: {4,8}, row 4: 4..8.
    #   row 1: A's 2..6: 2 has no B pixel within 1 (3 is not in B's row, rows 0 and 2 hold nothing at column 2) -> 3,4,5,6 match
    #          (3 is next to 4)                                                                                -> 4
    #   rows 2,3: A's 2: B has nothing at columns 1..3 of the row nor at column 2 of the rows above / below -> no;
    #             A's 6: B's row 1 / row 4 holds column 6 only next to rows 2 / 3... row 2's 6 is below row 1's 6 -> yes;
    #             row 3's 6 is above row 4's 6 -> yes                                                          -> 1 each
    #   row 4: as row 1                                                                                        -> 4
    # match_pred = 10; mirrored, match_gt = 10.
    b2 = rect(8, 12, 2, 5, 5, 9)
    assert list(M.jf_counts_numpy(a, b2, 1)) == [6, 18, 14, 14, 10, 10]


def ellipse_pair():
    y, x = np.mgrid[0:96, 0:160]
    a = ((y - 45) / 20) ** 2 + ((x - 80) / 26) ** 2 <= 1
    b = ((y - 47) / 19) ** 2 + ((x - 77) / 27) ** 2 <= 1
    return a, b


@pytest.mark.parametrize("radius,matches", [(1, (74, 71)), (2, (102, 102)), (8, (188, 188))])
def test_pinned_ellipse_pair(radius, matches):
    a, b = ellipse_pair()
    assert list(M.jf_counts_numpy(a, b, radius)) == [1457, 1773, 188, 188, matches[0], matches[1]]


def test_dilate_against_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.RandomState(3)
    for (h, w), r, density in [((40, 57), 1, 0.05), ((40, 57), 3, 0.01), ((64, 64), 8, 0.002), ((23, 130), 11, 0.003),
                               ((5, 7), 4, 0.2)]:
        m = rng.rand(h, w) < density
        yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
        want = ndimage.binary_dilation(m, structure=(yy * yy + xx * xx <= r * r))
        assert np.array_equal(M.dilate(m, r), want), (h, w, r)


def test_span_table_is_the_brute_force_disk():
    for r in range(1, 64):
        half = M.disk_half_widths(r)
        assert len(half) == 2 * r + 1
        spans = {(dy, dx) for dy, hw in zip(range(-r, r + 1), half) for dx in range(-hw, hw + 1)}
        assert spans == set(M.disk_offsets(r)), r
    assert M.disk_half_widths(8) == [0, 3, 5, 6, 6, 7, 7, 7, 8, 7, 7, 7, 6, 6, 5, 3, 0]


# ------------------------------------------------------------------------------------------ statistics
def test_sequence_statistics_hand_computed():
    # 11 frames, first and last dropped -> 0.9 .. 0.1 (n = 9); ids = round(linspace(1, 9, 5)) - 1 = [0, 2, 4, 6, 8]:
    # first quarter values[0:3] = .9 .8 .7 (mean .8), last quarter values[6:9] = .3 .2 .1 (mean .2)
    s = M.sequence_statistics([1.0, .9, .8, .7, .6, .5, .4, .3, .2, .1, 0.0])
    assert s["mean"] == pytest.approx(0.5) and s["recall"] == pytest.approx(4 / 9) and s["decay"] == pytest.approx(0.6)
    # 6 frames -> n = 4; linspace(1, 4, 5) = 1, 1.75, 2.5, 3.25, 4 -> round = 1 2 2 3 4 -> ids 0 1 1 2 3:
    # first quarter values[0:2] = .2 .4 (mean .3), last quarter values[2:4] = .6 .8 (mean .7)
    s = M.sequence_statistics([9, .2, .4, .6, .8, 9])
    assert s["mean"] == pytest.approx(0.5) and s["recall"] == pytest.approx(0.5) and s["decay"] == pytest.approx(-0.4)


def test_sequence_statistics_short_and_constant():
    s = M.sequence_statistics([0.25, 0.75])  # fewer than 3 frames: both count
    assert s["mean"] == pytest.approx(0.5) and s["recall"] == pytest.approx(0.5)
    assert s["decay"] == pytest.approx(-0.5)  # n = 2: ids = [0, 0, 0, 1, 1]: first quarter = [.25], last = [.75]
    s = M.sequence_statistics([0.6])
    assert s == {"mean": 0.6, "recall": 1.0, "decay": 0.0}
    s = M.sequence_statistics([0.0, 0.7, 1.0])  # 3 frames: only the middle one
    assert s == {"mean": 0.7, "recall": 1.0, "decay": 0.0}
    s = M.sequence_statistics([0.3] * 20)
    assert s["mean"] == pytest.approx(0.3) and s["recall"] == 0.0 and s["decay"] == 0.0


def test_default_radius():
    assert [M.default_radius(h, w) for h, w in [(480, 854), (384, 683), (240, 427), (1080, 1920), (61, 107)]] == \
        [8, 7, 4, 18, 1]


# ------------------------------------------------------------------------------------------ the scored pass on the CPU
class StandIn(torch.nn.Module):
    """Five maps derived from the input; the last one is the 'fused' logit map: positive on bright pixels."""

    def forward(self, x):
        base = x.mean(dim=1, keepdim=True)
        return [base * k for k in (0.1, 0.2, 0.3, 0.4)] + [(base - base.mean(dim=(1, 2, 3), keepdim=True)) * 0.05]


class Provider:
    def __init__(self):
        self.network = StandIn()


@pytest.fixture
def cpu_only(monkeypatch):
    # the pass moves its input with cast_cuda_if_possible; a stand-in network has no HIP path
    monkeypatch.setattr(experiment_helper.gpu_handler, "cast_cuda_if_possible", lambda ts, verbose=False: ts)


def expected_frame(net, image, gt, radius):
    x = net(image.unsqueeze(0))[-1][0, 0].numpy().astype(np.float64)
    png = experiment_helper.bytescale(1.0 / (1.0 + np.exp(-x)))
    return png, M.jf_counts_numpy(x >= 0, gt, radius)


def test_scored_pass_synthetic(tmp_path, cpu_only):
    loader = io_helper.get_data_loader_test(None, 2, "blob", synthetic=(40, 72), n_frames=5)
    prov = Provider()
    score = experiment_helper.test_scored(prov, loader, tmp_path, io_helper.get_annotations(None, loader, (40, 72)),
                                          seq_name="blob")
    assert score is not experiment_helper.last_score and score == experiment_helper.last_score
    assert score["fnames"] == ["%05d" % k for k in range(5)] and score["scored"] == [True] * 5
    assert score["radius"] == M.default_radius(40, 72) == 1
    assert sorted(p.name for p in (tmp_path / "blob").iterdir()) == ["%05d.png" % k for k in range(5)]
    counts = []
    for k in range(5):
        sample = loader.dataset[k]
        png, c = expected_frame(prov.network, sample["image"], sample["gt"][0].numpy() >= 0.5, 1)
        assert np.array_equal(np.asarray(Image.open(str(tmp_path / "blob" / ("%05d.png" % k)))), png)
        assert score["counts"][k] == list(c)
        counts.append(c)
    j, f = M.jf_from_counts(np.array(counts))
    assert score["J"] == list(j) and score["F"] == list(f)
    assert score["J_stats"] == M.sequence_statistics(j) and score["F_stats"] == M.sequence_statistics(f)
    assert score["J&F"] == (score["J_stats"]["mean"] + score["F_stats"]["mean"]) / 2
    assert 0.0 < score["J_stats"]["mean"] < 1.0  # the stand-in finds part of the bright object, not all of it

    experiment_helper.write_scores(tmp_path / "blob" / "scores.yml", score)
    assert yaml.safe_load((tmp_path / "blob" / "scores.yml").read_text()) == score

    # write_png=False: the same score, no files
    again = experiment_helper.test_scored(prov, loader, tmp_path / "none", loader.dataset.annotation, write_png=False,
                                          seq_name="blob")
    assert again["counts"] == score["counts"] and not (tmp_path / "none").exists()


def test_scored_pass_davis_tree(tmp_path, cpu_only):
    root = write_davis_tree(tmp_path / "davis")
    n, h, w = SEQS["bear"]
    loader = io_helper.get_data_loader_test(root, 1, "bear")
    loader = torch.utils.data.DataLoader(loader.dataset, batch_size=1, shuffle=False, num_workers=0)
    # the dataset hides every annotation but the first; the scorer reads the files itself
    assert [lab is not None for lab in loader.dataset.labels] == [True] + [False] * (n - 1)
    assert float(loader.dataset[1]["gt"].abs().max()) == 0.0
    # ... and one frame has none: it gets its PNG but no score
    (root / "Annotations" / "480p" / "bear" / "00001.png").unlink()
    annotations = io_helper.get_annotations(root, loader)
    assert annotations("bear", "00001") is None and annotations("bear", "00002").shape == (h, w)
    prov = Provider()
    score = experiment_helper.test_scored(prov, loader, tmp_path / "out", annotations, seq_name="bear")
    assert score["fnames"] == ["00000", "00001", "00002"] and score["scored"] == [True, False, True]
    assert score["counts"][1] is None and score["J"][1] is None and score["F"][1] is None
    assert sorted(p.name for p in (tmp_path / "out" / "bear").iterdir()) == ["00000.png", "00001.png", "00002.png"]
    r = M.default_radius(h, w)
    kept = []
    for k in (0, 2):
        mask = np.asarray(Image.open(str(root / "Annotations" / "480p" / "bear" / ("%05d.png" % k)))) >= 128
        assert mask.any() and np.array_equal(annotations("bear", "%05d" % k), mask.astype(np.uint8))
        png, c = expected_frame(prov.network, loader.dataset[k]["image"], mask, r)
        assert np.array_equal(np.asarray(Image.open(str(tmp_path / "out" / "bear" / ("%05d.png" % k)))), png)
        assert score["counts"][k] == list(c)
        kept.append(c)
    j, f = M.jf_from_counts(np.array(kept))
    assert score["J_stats"] == M.sequence_statistics(j) and score["F_stats"] == M.sequence_statistics(f)
    experiment_helper.write_scores(tmp_path / "out" / "bear" / "scores.yml", score)
    assert yaml.safe_load((tmp_path / "out" / "bear" / "scores.yml").read_text()) == score


def test_annotation_scale_is_per_frame(tmp_path):
    # write_davis_tree stores one mask as 0 / 7: normalised by its own maximum it is an object all the same
    root = write_davis_tree(tmp_path / "davis")
    ann = io_helper.get_annotations(root, None)("camel", "00001")
    raw = np.asarray(Image.open(str(root / "Annotations" / "480p" / "camel" / "00001.png")))
    assert raw.max() == 7 and np.array_equal(ann, (raw == 7).astype(np.uint8))


def test_scored_pass_rejects_a_wrong_sized_annotation(tmp_path, cpu_only):
    loader = io_helper.get_data_loader_test(None, 1, "blob", synthetic=(24, 40), n_frames=2)
    with pytest.raises(ValueError):
        experiment_helper.test_scored(Provider(), loader, tmp_path, lambda s, f: np.zeros((24, 41), dtype=np.uint8))


# ------------------------------------------------------------------------------------------ the flag
def test_score_flag():
    assert args_helper.parse_args(True, ["--synthetic"]).score is False
    assert args_helper.parse_args(True, ["--synthetic", "--score"]).score is True
    assert not hasattr(args_helper.parse_args(False, []), "score")
    with pytest.raises(SystemExit):
        args_helper.parse_args(False, ["--score"])


def test_score_with_eval_speeds_is_an_error():
    import train_online
    with pytest.raises(SystemExit):
        train_online.main(["--synthetic", "--score", "--eval-speeds"])
    assert train_online.score is False
