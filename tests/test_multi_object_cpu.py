"""Several objects a sequence, without a GPU: the numpy definitions the HIP kernels are tested against (util/object_merge.py,
``png_layout.encode_indexed``), the DAVIS 2017 dataset on a tree written with PIL, the host path of
``experiment_helper.test_objects`` and the parser's flag combinations."""
import io
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))

from util import args_helper, davis_measures as M, object_merge as OM, png_layout as P  # noqa: E402

NAN, INF = float("nan"), float("inf")


def blobs(h, w, k, seed=0):
    """A label map of k rectangles, some touching the frame edge, later ones on top."""
    rng = np.random.default_rng(seed)
    ids = np.zeros((h, w), dtype=np.uint8)
    for obj in range(1, k + 1):
        y0, x0 = int(rng.integers(0, max(h - 2, 1))), int(rng.integers(0, max(w - 2, 1)))
        ids[y0:y0 + int(rng.integers(2, h // 2 + 3)), x0:x0 + int(rng.integers(2, w // 2 + 3))] = obj
    return ids


# ------------------------------------------------------------------------------------------ merge_labels
def merge1(*columns):
    """merge_labels of K logits at each of several pixels: columns[p] = the K logits of pixel p."""
    x = np.array(columns, dtype=np.float32).T.reshape(len(columns[0]), 1, 1, len(columns))
    return OM.merge_labels(x)[0, 0].tolist()


def test_merge_labels_hand_made_cases():
    assert merge1((-1.0, -0.5, -3.0)) == [0]                       # all negative: background
    assert merge1((2.0, 5.0, 1.0), (0.5, -1.0, -2.0)) == [2, 1]
    assert merge1((-1.0, 3.0, 3.0), (3.0, 3.0, 3.0)) == [2, 1]     # a tie: the lowest id
    assert merge1((-1.0, -0.0, -2.0)) == [2]                       # -0.0 is valid, as in `logit >= 0`
    assert merge1((0.0, -0.0), (-0.0, 0.0)) == [1, 1]              # ... and equal to +0.0
    assert merge1((NAN, 1.0), (1.0, NAN), (NAN, NAN), (NAN, -1.0)) == [2, 1, 0, 0]   # a NaN is never valid
    assert merge1((1.0, INF, INF), (-INF, -INF, -INF), (INF, 5.0, NAN)) == [2, 0, 1]  # +inf twice: the lowest id
    rng = np.random.default_rng(0)
    x = rng.normal(size=(1, 2, 7, 9)).astype(np.float32)
    x[0, 0, 0, :3] = [0.0, -0.0, NAN]
    assert np.array_equal(OM.merge_labels(x), (x[0] >= 0).astype(np.uint8))          # K = 1: the existing mask
    # K arrays [N,H,W] are taken like one [K,N,H,W]
    y = rng.normal(size=(3, 2, 7, 9)).astype(np.float32)
    assert np.array_equal(OM.merge_labels(list(y)), OM.merge_labels(y)) and OM.merge_labels(y).dtype == np.uint8
    for bad in (np.zeros((0, 1, 2, 2), np.float32), np.zeros((17, 1, 2, 2), np.float32), np.zeros((2, 2, 2), np.float32)):
        with pytest.raises(ValueError):
            OM.merge_labels(bad)


def test_merge_labels_is_the_plain_rule_on_random_logits():
    rng = np.random.default_rng(3)
    x = rng.normal(size=(5, 2, 6, 11)).astype(np.float32)
    x[rng.random(x.shape) < 0.1] = 1.5           # planted ties
    x[rng.random(x.shape) < 0.05] = NAN
    got = OM.merge_labels(x)
    for n, yy, xx in np.ndindex(got.shape):
        best, bestv = 0, None
        for k in range(x.shape[0]):
            v = x[k, n, yy, xx]
            if v >= 0 and (bestv is None or v > bestv):
                best, bestv = k + 1, v
        assert got[n, yy, xx] == best


# ------------------------------------------------------------------------------------------ counts per object
def test_jf_counts_labels_numpy():
    pred, gt = blobs(24, 40, 3, seed=1), blobs(24, 40, 3, seed=2)
    pred[2:5, 30:38] = 9                          # an id above K belongs to no object
    got = OM.jf_counts_labels_numpy(pred, gt, 3, 2)
    assert got.shape == (3, 6) and got.dtype == np.int64
    for k in (1, 2, 3):
        assert np.array_equal(got[k - 1], M.jf_counts_numpy(pred == k, gt == k, 2))
    clean = pred.copy()
    clean[pred == 9] = 0
    assert np.array_equal(got, OM.jf_counts_labels_numpy(clean, gt, 3, 2))
    # an object absent from both maps: J = F = 1
    five = OM.jf_counts_labels_numpy(pred, gt, 5, 2)
    assert np.array_equal(five[:3], got) and not five[3:].any()
    j, f = M.jf_from_counts(five)
    assert j[3] == f[3] == j[4] == f[4] == 1.0
    with pytest.raises(ValueError):
        OM.jf_counts_labels_numpy(pred, gt, 0, 2)
    with pytest.raises(ValueError):
        OM.jf_counts_labels_numpy(pred, gt[:-1], 3, 2)


# ------------------------------------------------------------------------------------------ palette and palette files
def test_davis_palette():
    pal = OM.davis_palette()
    assert pal.shape == (256, 3) and pal.dtype == np.uint8
    assert pal[:4].tolist() == [[0, 0, 0], [128, 0, 0], [0, 128, 0], [128, 128, 0]]
    assert pal[4:9].tolist() == [[0, 0, 128], [128, 0, 128], [0, 128, 128], [128, 128, 128], [64, 0, 0]]
    assert pal[255].tolist() == [224, 224, 192] and len({tuple(c) for c in pal.tolist()}) == 256
    # through a file PIL itself wrote
    im = Image.fromarray(blobs(8, 8, 3), mode="P")
    im.putpalette(pal.tobytes())
    buf = io.BytesIO()
    im.save(buf, format="PNG")
    back = Image.open(io.BytesIO(buf.getvalue()))
    assert back.mode == "P" and np.array_equal(np.array(back.getpalette(), dtype=np.uint8).reshape(-1, 3), pal)


INDEXED_CASES = {
    "8x8_flat": np.full((8, 8), 2, dtype=np.uint8),
    "64x64_blobs": blobs(64, 64, 3, seed=4),
    "65x67_blobs": blobs(65, 67, 5, seed=5),
    "65x67_noise": np.random.default_rng(6).integers(0, 4, (65, 67), dtype=np.uint8),
    "96x160_blobs": blobs(96, 160, 16, seed=7),
}


@pytest.mark.parametrize("huffman", P.HUFFMAN_MODES)
@pytest.mark.parametrize("name", list(INDEXED_CASES))
def test_encode_indexed(name, huffman):
    labels = INDEXED_CASES[name]
    h, w = labels.shape
    for palette in (None, np.random.default_rng(8).integers(0, 256, (256, 3), dtype=np.uint8)):
        file = P.encode_indexed(labels, palette, huffman=huffman)
        want_palette = OM.davis_palette() if palette is None else palette
        im = Image.open(io.BytesIO(file))
        im.load()
        assert im.mode == "P" and np.array_equal(np.asarray(im), labels)
        assert np.array_equal(np.array(im.getpalette(), dtype=np.uint8).reshape(-1, 3), want_palette)
        got, grey = P.chunks(file), P.chunks(P.encode(labels, huffman))
        assert [t for t, _ in got] == [b"IHDR", b"PLTE"] + [b"IDAT"] * (P.n_segments(h, w) + 1) + [b"IEND"]
        assert got[0][1] == grey[0][1][:9] + b"\x03" + grey[0][1][10:] and got[0][1][8] == 8
        assert got[1][1] == want_palette.tobytes() and len(got[1][1]) == 768
        assert got[2:] == grey[1:]                 # every IDAT, and IEND, are the greyscale file's
        assert len(file) == len(P.encode(labels, huffman)) + 780 <= P.max_file_bytes_indexed(h, w)
    assert P.max_file_bytes_indexed(h, w) == P.max_file_bytes(h, w) + 780
    with pytest.raises(ValueError):
        P.encode_indexed(labels, np.zeros((16, 3), dtype=np.uint8))


def test_second_segment_of_64x64_is_64_bytes():
    assert 64 * 65 == 4160 and P.n_segments(64, 64) == 2 and P.n_segments(8, 8) == 1 and P.n_segments(65, 67) == 2


# ------------------------------------------------------------------------------------------ DAVIS 2017 on disk
def write_tree(root):
    """Two sequences of 24x40 frames: 'one' with 1 object (3 frames), 'three' with 3 objects (2 frames)."""
    pal = OM.davis_palette()
    rng = np.random.default_rng(9)
    ids = {}
    (root / "ImageSets" / "2017").mkdir(parents=True)
    (root / "ImageSets" / "2017" / "train.txt").write_text("one\n")
    (root / "ImageSets" / "2017" / "val.txt").write_text("three\n")
    for seq, k, n in (("one", 1, 3), ("three", 3, 2)):
        (root / "JPEGImages" / "480p" / seq).mkdir(parents=True)
        (root / "Annotations" / "480p" / seq).mkdir(parents=True)
        for f in range(n):
            Image.fromarray(rng.integers(0, 256, (24, 40, 3), dtype=np.uint8)).save(
                str(root / "JPEGImages" / "480p" / seq / ("%05d.jpg" % f)), quality=95)
            m = np.zeros((24, 40), dtype=np.uint8)
            for obj in range(1, k + 1):
                m[2 + 5 * obj + f:9 + 5 * obj + f, 3 + 8 * obj:14 + 8 * obj] = obj
            im = Image.fromarray(m, mode="P")
            im.putpalette(pal.tobytes())
            im.save(str(root / "Annotations" / "480p" / seq / ("%05d.png" % f)))
            ids[(seq, "%05d" % f)] = m
    return ids


def test_davis_2017_dataset(tmp_path):
    from dataloaders import davis_2017 as D
    from dataloaders.davis_2016 import DAVIS2016, read_bgr
    from dataloaders.resident import ResidentOneShotLoader
    ids = write_tree(tmp_path)
    assert D.sequence_names(tmp_path, "train") == ["one"] and D.sequence_names(tmp_path, "val") == ["three"]
    assert D.n_objects(tmp_path, "one") == 1 and D.n_objects(tmp_path, "three") == 3
    ann = D.Davis2017Annotations(tmp_path)
    for (seq, fname), m in ids.items():
        got = ann(seq, fname)
        assert got.dtype == np.uint8 and np.array_equal(got, m)      # the ids survive: no palette colours, no luminance
    assert ann("three", "00007") is None
    for obj in (1, 2, 3):
        test_set = D.DAVIS2017("test", tmp_path, "three", obj)
        assert isinstance(test_set, DAVIS2016) and len(test_set) == 2
        assert test_set.fname_list == ["00000", "00001"] and test_set.seq_list == ["three"] * 2
        first, second = test_set[0], test_set[1]
        assert first["gt"].dtype == np.float32 and np.array_equal(first["gt"], (ids[("three", "00000")] == obj))
        assert not second["gt"].any() and second["gt"].shape == (24, 40)     # hidden after frame 0
        frame = read_bgr(str(tmp_path / "JPEGImages" / "480p" / "three" / "00000.jpg")).astype(np.float32)
        assert np.array_equal(first["image"], frame - np.asarray(D.MEANVAL, dtype=np.float32))
        train_set = D.DAVIS2017("train", tmp_path, "three", obj)
        assert len(train_set) == 1 and np.array_equal(train_set[0]["gt"], first["gt"])
    assert len(D.DAVIS2017("test", tmp_path, "one", 1)) == 3
    for bad in (0, 4):
        with pytest.raises(ValueError):
            D.DAVIS2017("train", tmp_path, "three", bad)
    with pytest.raises(RuntimeError):
        D.DAVIS2017("train", tmp_path, "nowhere", 1)
    # a greyscale annotation is taken as ids too
    Image.fromarray(ids[("three", "00000")], mode="L").save(str(tmp_path / "Annotations" / "480p" / "three" / "00000.png"))
    assert np.array_equal(ann("three", "00000"), ids[("three", "00000")]) and D.n_objects(tmp_path, "three") == 3

    # the resident one-shot loader yields the plain loader's sample (same seed: same flip and scale)
    from dataloaders import custom_transforms
    from torch.utils.data import DataLoader
    composed = custom_transforms.Compose([custom_transforms.RandomHorizontalFlip(), custom_transforms.Resize(),
                                          custom_transforms.ToTensor()])
    plain = DataLoader(D.DAVIS2017("train", tmp_path, "three", 2, transform=composed), batch_size=1, shuffle=True,
                       num_workers=1)
    resident = ResidentOneShotLoader(D.DAVIS2017("train", tmp_path, "three", 2), device=torch.device("cpu"))
    for seed in (0, 1, 2):
        torch.manual_seed(seed)
        want = next(iter(plain))
        torch.manual_seed(seed)
        got = next(iter(resident))
        assert torch.equal(got["image"], want["image"]) and torch.equal(got["gt"], want["gt"])
        assert got["fname"] == want["fname"] and got["seq_name"] == want["seq_name"]
        assert set(got["gt"].unique().tolist()) <= {0.0, 1.0} and got["gt"].any()


def test_synthetic_objects_sequence():
    from dataloaders.synthetic import SyntheticObjectsSequence, SyntheticSequence
    seq = SyntheticObjectsSequence("blobs", 48, 80, n_frames=3, n_objects=3, seed=5)
    maps = [seq.annotation("blobs", "%05d" % k) for k in range(3)]
    assert all(m.dtype == np.uint8 and m.shape == (48, 80) and set(np.unique(m)) == {0, 1, 2, 3} for m in maps)
    assert not np.array_equal(maps[0], maps[1])                     # the centres drift
    assert seq.annotation("blobs", "00003") is None and seq.annotation("other", "00000") is None
    sample = seq[1]
    assert sample["image"].shape == (3, 48, 80) and sample["fname"] == "00001" and sample["seq_name"] == "blobs"
    assert np.array_equal(sample["gt"][0].numpy(), (maps[1] != 0))
    for k in (1, 2, 3):
        one = SyntheticObjectsSequence("blobs", 48, 80, n_frames=1, n_objects=3, object_id=k, seed=5)[0]
        assert np.array_equal(one["gt"][0].numpy(), (maps[0] == k)) and torch.equal(one["image"], seq[0]["image"])
    # the objects differ in colour
    means = [seq[0]["image"][:, torch.from_numpy(maps[0] == k)].mean(dim=1) for k in (1, 2, 3)]
    assert all((means[a] - means[b]).abs().max() > 20 for a in range(3) for b in range(a))
    # higher ids lie on top where two ellipses overlap
    wide = SyntheticObjectsSequence("w", 48, 80, n_frames=7, n_objects=16)
    assert set(np.unique(wide.annotation("w", "00006"))) == set(range(17))
    with pytest.raises(ValueError):
        SyntheticObjectsSequence(n_objects=17)
    with pytest.raises(ValueError):
        SyntheticObjectsSequence(n_objects=2, object_id=3)
    assert SyntheticSequence("s", 8, 8)[0]["gt"].shape == (1, 8, 8)


# ------------------------------------------------------------------------------------------ the test pass, host path
class Net:
    """A CPU stand-in: the frame's channel ``channel``, centred, plus seeded noise."""

    def __init__(self, channel, seed):
        self.channel, self.seed = channel, seed

    def forward(self, x):
        x = x.cpu()  # (the pass forwards two frames a call: every frame draws its own noise, whatever batch it comes in)
        c = x[:, self.channel:self.channel + 1]
        base = (c - c.flatten(1).median(dim=1).values.view(-1, 1, 1, 1)) / 8
        noise = [torch.randn(f.shape, generator=torch.Generator().manual_seed(self.seed + int(f.abs().sum() * 10) % 1000))
                 for f in base]
        return [base + 0.5 * torch.stack(noise)]


class Provider:
    def __init__(self, network):
        self.network = network


@pytest.mark.parametrize("huffman", P.HUFFMAN_MODES)
def test_objects_pass_host_path(tmp_path, huffman):
    from dataloaders.synthetic import SyntheticObjectsSequence
    from torch.utils.data import DataLoader
    from util import experiment_helper
    data = SyntheticObjectsSequence("blobs", 24, 40, n_frames=7, n_objects=3)
    loader = DataLoader(data, batch_size=1, shuffle=False, num_workers=0)
    providers = [Provider(Net(k, 10 + k)) for k in range(3)]
    palette = np.random.default_rng(1).integers(0, 256, (256, 3), dtype=np.uint8) if huffman == "fitted" else None
    score = experiment_helper.test_objects(providers, loader, tmp_path, data.annotation, seq_name="blobs",
                                           png_huffman=huffman, palette=palette)
    assert score == experiment_helper.last_score
    names = sorted(p.name for p in (tmp_path / "blobs").iterdir())
    assert names == ["%05d.png" % k for k in range(7)]
    radius = M.default_radius(24, 40)
    counts = np.zeros((7, 3, 6), dtype=np.int64)
    for k in range(7):
        image = data[k]["image"][None]
        want = OM.merge_labels([p.network.forward(image)[-1][:, 0].numpy() for p in providers])[0]
        im = Image.open(str(tmp_path / "blobs" / names[k]))
        assert im.mode == "P" and np.array_equal(np.asarray(im), want)
        assert (tmp_path / "blobs" / names[k]).read_bytes() == P.encode_indexed(want, palette, huffman)
        assert len(set(np.unique(want))) > 1
        counts[k] = OM.jf_counts_labels_numpy(want, data.annotation("blobs", "%05d" % k), 3, radius)
    assert score["seq_name"] == "blobs" and score["radius"] == radius and score["n_objects"] == 3
    assert score["fnames"] == ["%05d" % k for k in range(7)] and score["scored"] == [True] * 7
    assert [o["object_id"] for o in score["objects"]] == [1, 2, 3]
    for k, obj in enumerate(score["objects"]):
        j, f = M.jf_from_counts(counts[:, k])
        assert obj["counts"] == counts[:, k].tolist() and obj["J"] == list(j) and obj["F"] == list(f)
        assert obj["J_stats"] == M.sequence_statistics(j) and obj["F_stats"] == M.sequence_statistics(f)
    for name in ("J_stats", "F_stats"):
        for stat in ("mean", "recall", "decay"):
            assert score[name][stat] == pytest.approx(np.mean([o[name][stat] for o in score["objects"]]), abs=1e-15)
    assert score["J&F"] == (score["J_stats"]["mean"] + score["F_stats"]["mean"]) / 2 and score["seconds"] > 0
    # the dict goes through the writer and the formatter
    import yaml
    experiment_helper.write_scores(tmp_path / "scores.yml", score)
    back = yaml.safe_load((tmp_path / "scores.yml").read_text())
    assert len(back["objects"]) == 3 and back["objects"][1]["counts"] == score["objects"][1]["counts"]
    assert "3 objects" in experiment_helper.format_score(score)
    # without annotations: files, no score
    assert experiment_helper.test_objects(providers[:2], loader, tmp_path / "plain", seq_name="blobs") is None
    assert len(list((tmp_path / "plain" / "blobs").iterdir())) == 7
    with pytest.raises(ValueError):
        experiment_helper.test_objects([], loader, tmp_path / "bad")
    with pytest.raises(ValueError):
        experiment_helper.test_objects(providers, loader, tmp_path / "bad", png_huffman="best")


# ------------------------------------------------------------------------------------------ the parser
def test_multi_object_flag_combinations():
    args = args_helper.parse_args(True, ["--synthetic", "--multi-object"])
    assert args.multi_object and args.objects == 2 and not args.score
    assert args_helper.parse_args(True, ["--synthetic", "--multi-object", "--objects", "5"]).objects == 5
    assert not args_helper.parse_args(True, ["--synthetic"]).multi_object
    args = args_helper.parse_args(True, ["--synthetic", "--multi-object", "--score", "--png-fitted"])   # no --fast-test needed
    assert args.score and args.png_fitted and not args.fast_test
    assert args_helper.parse_args(True, ["--multi-object", "--score", "--fast-test", "--png-fitted"]).multi_object
    for bad in (["--eval-speeds"], ["--data-parallel"], ["--objects", "0"], ["--objects", "17"]):
        with pytest.raises(SystemExit):
            args_helper.parse_args(True, ["--synthetic", "--multi-object"] + bad)
    with pytest.raises(SystemExit):
        args_helper.parse_args(True, ["--synthetic", "--png-fitted"])         # still needs --fast-test on its own
    with pytest.raises(SystemExit):
        args_helper.parse_args(False, ["--synthetic", "--multi-object"])      # an online flag


def test_rejections_name_their_reason(capsys):
    for flag, word in (("--eval-speeds", "writes nothing"), ("--data-parallel", "one device")):
        with pytest.raises(SystemExit):
            args_helper.parse_args(True, ["--synthetic", "--multi-object", flag])
        assert word in capsys.readouterr().err
